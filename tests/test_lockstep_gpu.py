"""Fit groups with a consumer, on the GPU: the group's host path in two halves on mapped memory (tamcmc_group_eval_begin /
_end / _poll), samplers driven through a lockstep object over a group, and the command-line mode that runs the slices of
a local fit together.  Group results are bitwise the solo results, so every comparison here is of bits, over the whole
run: no tolerance and no prefix."""
import ctypes as C
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

import test_group_gpu as tg
import workloads as W
from tamcmc_amd import capi
from tamcmc_amd import sampler as S
from tamcmc_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = ("vars", "logL", "sigma", "mu", "covarmat")
JOIN_TIMEOUT = 240.0


def mixed_members(accel_mod):
    """(name, Accel, P, T): multi-tile members, a one-tile (fused) member, two on the generic body (chi_square, id 1), one
    with a NaN chain and an empty window, and one that always sits out.  The launch geometry is whatever the developer
    switches in force make it (tools/modes_check.sh): the bits must agree under all of them."""
    out = []
    w = synth.workload_c2(Nx=100000)
    acc = accel_mod.Accel(2, w["plength"], w["x"], tg._spectrum(2, w, 1))
    assert acc.geometry()["tiles"] > 1
    out.append(("id2-1e5", acc, synth.chain_params(w, 12), synth.temperatures(12)))
    w = W.make(3, Nx=30000)
    out.append(("id3", accel_mod.Accel(3, w["plength"], w["x"], tg._spectrum(3, w, 2)), W.perturbed(w, 5, seed=5), np.linspace(1.0, 4.0, 5)))
    w = W.any_model(9, Nx=9000)
    off = np.concatenate([[0], np.cumsum(np.asarray(w["plength"]))])
    base = np.asarray(w["params_true"], dtype=float)
    P = np.tile(base, (4, 1))
    P[1, off[7] + 1] = base[off[7]]        # the width overflows -> status 1
    P[2, off[7]] = -base[off[7]]           # negative width -> empty truncation window, status 2
    P[3] = W.perturbed(w, 2, seed=9)[1]
    out.append(("id9-special", accel_mod.Accel(9, w["plength"], w["x"], tg._spectrum(9, w, 3)), P, np.array([1.0, 1.5, 2.0, 2.5])))
    w = W.any_model(14, Nx=3000)
    out.append(("id14", accel_mod.Accel(14, w["plength"], w["x"], tg._spectrum(14, w, 4)), W.perturbed(w, 6, seed=6), np.linspace(1.0, 2.0, 6)))
    w = W.make(2, Nx=8000)
    y = tg._spectrum(2, w, 5)
    out.append(("chi2", accel_mod.Accel(2, w["plength"], w["x"], y, sigma_y=0.1 + 0.05 * np.abs(y), likelihood_case=1),
                W.perturbed(w, 5, seed=7), np.linspace(1.0, 3.0, 5)))
    w = W.any_model(1, Nx=4096)
    out.append(("id1", accel_mod.Accel(1, w["plength"], w["x"], tg._spectrum(1, w, 6)), W.perturbed(w, 3, seed=8), np.array([1.0, 1.3, 1.9])))
    w = W.any_model(11, Nx=2000)
    acc = accel_mod.Accel(11, w["plength"], w["x"], tg._spectrum(11, w, 8))
    assert acc.geometry()["tiles"] == 1
    out.append(("one-tile", acc, W.perturbed(w, 3, seed=10), np.array([1.0, 1.4, 2.0])))
    w = W.any_model(12, Nx=5000)
    out.append(("idle", accel_mod.Accel(12, w["plength"], w["x"], tg._spectrum(12, w, 9)), np.empty((0, int(np.sum(w["plength"])))), np.empty(0)))
    return out


def _poll_all(g, counts):
    """One look at every slot of the batch in flight: None (pending) or (logL, status); anything else raises."""
    seen = {}
    for k, n in enumerate(counts):
        for c in range(n):
            r = g.poll(k, c)
            if r is not None:
                seen[(k, c)] = r
    return seen


def test_begin_end_return_the_bits_of_the_group_call_and_of_every_member_alone(accel_mod):
    mem = mixed_members(accel_mod)
    names = [m[0] for m in mem]
    accels = [m[1] for m in mem]
    assert {"id2-1e5", "one-tile", "chi2", "id1"} <= set(names)        # multi-tile, fused, and the generic body twice
    full = [len(m[2]) for m in mem]
    rng = np.random.default_rng(4)
    solo = {}

    def solo_bits(k, P, T):
        key = (k, len(P))
        if key not in solo:
            solo[key] = accels[k].eval_batch(P, T)
        return solo[key]

    with accel_mod.Group(accels) as g:
        for call in range(7):
            # chain counts change from call to call; a member that normally takes part sits some calls out
            counts = [n if call == 0 else int(rng.integers(0, n + 1)) for n in full]
            if call == 3:
                counts[names.index("id3")] = 0
            if sum(counts) == 0:
                counts[0] = 1
            P_list = [m[2][:n] for m, n in zip(mem, counts)]
            T_list = [m[3][:n] for m, n in zip(mem, counts)]
            g.begin(P_list, T_list)
            seen = _poll_all(g, counts)                                # (what has arrived must be final)
            L, st = g.end()
            for (k, c), (lv, sv) in seen.items():
                assert tg.bits_equal([lv], [L[k][c]]) and sv == st[k][c], (call, k, c)
            L2, st2 = g.eval(P_list, T_list)                            # the existing host path
            for k, n in enumerate(counts):
                assert L[k].shape == (n,) and st[k].shape == (n,)
                assert tg.bits_equal(L[k], L2[k]) and np.array_equal(st[k], st2[k]), (call, names[k])
                if n == 0:
                    continue
                # a solo call on the member, right behind the group calls and without any synchronisation by the test
                rL, rst = accels[k].eval_batch(P_list[k], T_list[k]) if call % 2 == 0 else solo_bits(k, P_list[k], T_list[k])
                assert tg.bits_equal(L[k], rL) and np.array_equal(st[k], rst), (call, names[k])
            # two batches back to back with solo calls of two members between them (begin / end of the member itself)
            if call == 5:
                g.begin(P_list, T_list)
                La, sta = g.end()
                j = names.index("id14")
                accels[j].begin(mem[j][2], mem[j][3])
                sL, sst = accels[j].end()
                g.begin(P_list, T_list)
                Lb, stb = g.end()
                for k in range(len(mem)):
                    assert tg.bits_equal(La[k], L[k]) and tg.bits_equal(Lb[k], L[k])
                    assert np.array_equal(sta[k], st[k]) and np.array_equal(stb[k], st[k])
                rL, rst = accels[j].eval_batch(mem[j][2], mem[j][3])
                assert tg.bits_equal(sL, rL) and np.array_equal(sst, rst)
        k = names.index("id9-special")
        g.begin([m[2] for m in mem], [m[3] for m in mem])
        L, st = g.end()
        assert list(st[k]) == [0, capi.CHAIN_NAN, capi.CHAIN_EMPTY_WINDOW, 0]
    tg.close_all(mem)


def test_misuse_of_the_two_halves_is_refused_and_the_group_works_afterwards(accel_mod):
    mem = [m for m in mixed_members(accel_mod) if m[0] in ("id3", "id14", "one-tile")]
    accels = [m[1] for m in mem]
    P_list, T_list = [m[2] for m in mem], [m[3] for m in mem]
    lib = capi.load_library()
    n = np.array([len(p) for p in P_list], dtype=np.int32)
    tot = int(n.sum())
    buf, ist = np.empty(tot), np.empty(tot, dtype=np.int32)
    Lone, sone = C.c_double(), C.c_int32()
    g = accel_mod.Group(accels)
    ref = g.eval(P_list, T_list)

    def refused(fn, *a):
        with pytest.raises(capi.AccelError) as e:
            fn(*a)
        assert e.value.code == capi.E_INVALID

    refused(g.end)                                                       # _end without _begin
    assert lib.tamcmc_group_eval_poll(g._g, 0, 0, C.byref(Lone), C.byref(sone)) == capi.E_INVALID   # nothing in flight
    assert lib.tamcmc_group_eval_begin(None, capi._iptr(n), capi._iptr(g.Nparams), capi._dptr(buf), capi._dptr(buf)) == capi.E_INVALID
    assert lib.tamcmc_group_eval_begin(g._g, capi._iptr(n), capi._iptr(g.Nparams), None, capi._dptr(buf)) == capi.E_INVALID
    g.begin(P_list, T_list)
    refused(g.begin, P_list, T_list)                                     # a second _begin
    refused(g.eval, P_list, T_list)                                      # tamcmc_group_eval while a batch is in flight
    refused(g.synchronize)
    refused(g.set_stream, 0)
    assert lib.tamcmc_group_eval_end(g._g, None, capi._iptr(ist)) == capi.E_INVALID                 # (and the batch stays in flight)
    for member, chain in ((-1, 0), (len(mem), 0), (0, -1), (0, int(n[0])), (2, int(n[2]))):
        assert lib.tamcmc_group_eval_poll(g._g, member, chain, C.byref(Lone), C.byref(sone)) == capi.E_INVALID
    L, st = g.end()
    refused(g.end)
    for k in range(len(mem)):
        assert tg.bits_equal(L[k], ref[0][k]) and np.array_equal(st[k], ref[1][k])
    # a member with a solo batch in flight, a member that is armed
    accels[0].begin(P_list[0], T_list[0])
    refused(g.begin, P_list, T_list)
    accels[0].end()
    accels[1].arm(len(P_list[1]))
    refused(g.begin, P_list, T_list)
    accels[1].disarm()
    g.begin(P_list, T_list)
    L, st = g.end()
    for k in range(len(mem)):
        assert tg.bits_equal(L[k], ref[0][k]) and np.array_equal(st[k], ref[1][k])
    # destroy with a batch in flight: returns after draining, and the members are free again
    g.begin(P_list, T_list)
    g.close()
    for a, P, T, l in zip(accels, P_list, T_list, ref[0]):
        assert tg.bits_equal(a.eval_batch(P, T)[0], l)
        a.close()


# ---------------------------------------------------------------------------------------------------------------------
def _slice_sampler(s, nch, Nt_learn, evaluator=None, lockstep=None):
    cfg = s.sampler_cfg(seed=42)
    cfg.Nchains = cfg.Nchains_local = nch
    cfg.lambda_temp = 1.7
    cfg.dN_mixing = 1
    cfg.n_learn = 3
    for i, v in enumerate(Nt_learn):
        cfg.Nt_learn[i] = v
    cfg.periods_learn[0] = cfg.periods_learn[1] = 1
    return S.Sampler(cfg, evaluator, s.plength, s.inputs, s.relax, s.err, s.priors_names_switch, s.priors, s.extra_priors,
                     lockstep=lockstep)


def _walk(smp, stretches, every):
    smp.init()
    out = []
    for n in stretches:
        done = 0
        while done < n:
            mv, sw = smp.run(min(every, n - done))
            out.append((mv, sw, {name: smp.get(name).copy() for name in STATE}))
            done += min(every, n - done)
    return out


def test_the_eight_slices_in_lockstep_walk_their_solo_paths(accel_mod):
    """One sampler per slice of the reference's local example through tamcmc_lockstep_create_group, against the same
    samplers alone on tamcmc_sampler_create_hip: a stretch with the proposal adapting on every iteration (Burn-in like), then
    one with the proposal frozen (Acquire like), 500 iterations each, checkpoints every 100."""
    sl = [s for s, _, _ in tg.slices()]
    assert len(sl) == 8
    nch, n_adapt, n_frozen = 10, 500, 500
    learn = (0, n_adapt, n_adapt + 1)                     # adapting on iterations [0, 500), frozen afterwards
    accels = [tg.slice_accel(accel_mod, s) for s in sl]
    alone = []
    for s, acc in zip(sl, accels):
        smp = _slice_sampler(s, nch, learn, evaluator=acc)
        alone.append(_walk(smp, (n_adapt, n_frozen), 100))
        smp.close()
    with accel_mod.Group(accels) as g:
        ls = S.Lockstep(g)
        smps = [_slice_sampler(s, nch, learn, lockstep=(ls, k)) for k, s in enumerate(sl)]
        for k in range(8):
            ls.join(k)
        together, errs = [None] * 8, []

        def work(k):
            try:
                together[k] = _walk(smps[k], (n_adapt, n_frozen), 100)
            except BaseException as e:       # noqa: BLE001
                errs.append(e)
            finally:
                ls.leave(k)
        th = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(8)]
        for t in th:
            t.start()
        for t in th:
            t.join(JOIN_TIMEOUT)
        assert not any(t.is_alive() for t in th), "a sampler thread did not end"
        assert not errs, (errs, ls.error())
        assert ls.calls() == n_adapt + n_frozen + 1      # full rounds: one launch set per iteration for all eight
        for s in smps:
            s.close()
        ls.close()
    for k in range(8):
        assert len(alone[k]) == len(together[k]) == 10
        moves = 0.0
        for (mv, sw, st), (mv2, sw2, st2) in zip(alone[k], together[k]):
            assert np.array_equal(mv, mv2) and np.array_equal(sw, sw2), k
            for name in STATE:
                assert np.array_equal(st[name].view(np.int64), st2[name].view(np.int64)), (k, name)
            moves += mv.mean()
        assert moves > 0.2, k                             # (chains do move)
    for a in accels:
        a.close()


PRESETS = """
   force_manual_config=0;
   manual_config_file=;
   cfg_models_dir={G}/;
   cfg_out_dir={out};
   processing      = Burn-in  , Learning , Acquire;
   Nsamples        = 600     ,  400  , 500;
   c0              = 1.8      ,   1.7   ,    0;
   restore         =  0       ,    1    ,    2;
   core_out        =  B       ,    L    ,    A;
   core_in         =  B       ,    B    ,    L;
   start_index_processing=0;
   last_index_processing=2;
   table_ids=1, 2;
TF_3443483_local-v3   1;
/END;
"""


def test_command_line_together_writes_the_files_of_the_sequential_run(tmp_path):
    """Slices 1-4, the short three-phase recipe of test_cli_gpu: every file under outputs/ and restore/ byte for byte."""
    exe = os.path.join(ROOT, "bin", "cpptamcmc_hip")
    trees = {}
    for tag, flags in (("seq", []), ("tog", ["--together"])):
        root = tmp_path / tag / "run"
        shutil.copytree(tg.CFG, root / "Config" / "default")
        path = root / "Config" / "default" / "config_default.cfg"
        cfg = open(path).read()
        cfg = cfg.replace("Nchains=10;", "Nchains=6;").replace("Nbuffer=10000;", "Nbuffer=250;").replace("Nt_learn=500, 1500, 100000;", "Nt_learn=50, 150, 100000;")
        open(path, "w").write(cfg)
        out = tmp_path / tag / "out"
        open(root / "Config" / "config_presets.cfg", "w").write(PRESETS.format(G=tg.G, out=out))
        # (first slice 1-based inclusive, last exclusive after the -1 shift: "1 5" runs the slices numbered 1 to 4)
        r = subprocess.run([exe, "execute", "1", "1", "1", "1", "5", "--root", str(root), "--seed", "42", "--quiet"] + flags,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert ("Frequency Slices 1-4/8 together" in r.stdout) == bool(flags)
        trees[tag] = out / "TF_3443483_local-v3"
    for sub in ("outputs", "restore"):
        a, b = sorted(os.listdir(trees["seq"] / sub)), sorted(os.listdir(trees["tog"] / sub))
        assert a == b and len(a) >= 4 * 3 * 3
        for name in a:
            assert open(trees["seq"] / sub / name, "rb").read() == open(trees["tog"] / sub / name, "rb").read(), (sub, name)
    # an object with one slice selected runs as without the flag
    root = tmp_path / "tog" / "run"
    r = subprocess.run([exe, "execute", "1", "1", "1", "2", "3", "--root", str(root), "--seed", "42", "--quiet", "--together"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Frequency Slice 2/8 " in r.stdout and "Frequency Slices" not in r.stdout
