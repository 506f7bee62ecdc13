"""The lockstep evaluator on the CPU (include/tamcmc_sampler.h, tamcmc_lockstep_*): K samplers on K threads share one
backend call per iteration.  The backend here is a Python callable that evaluates each member with the oracle, so a
sampler driven through the object must walk, bit for bit, the path of the same sampler run alone through
tamcmc_sampler_create with the oracle: identical moved / swap histories over the whole run, identical vars, tempered
logL, sigma, mu and covarmat at every checkpoint.  No tolerance anywhere."""
import ctypes as C
import threading

import numpy as np

import test_priors_sampler as tps
import workloads as W
from tamcmc_amd import capi
from tamcmc_amd import sampler as S
from tamcmc_amd import synth

STATE = ("vars", "logL", "sigma", "mu", "covarmat")
JOIN_TIMEOUT = 300.0          # seconds; a deadlock check, not a timing


def fits(orc):
    """Three fits that differ in model id, chain count and parameter count."""
    out = []
    w, sw, pp, _ = tps.ms_global_prior_setup()
    w = dict(w); w["x"] = synth.grid(800, 2300.0, 840.0 / 800)
    m, _ = orc.model(3, w["params_true"], w["plength"], w["x"])
    out.append(dict(mid=3, w=w, y=synth.make_spectrum(m, seed=5), nch=4, err=w["err"], sw=sw, pp=pp, extra=[1.0, 5.0, 0.5, 0.0],
                    prior=2, seed=11))
    for mid, nx, nch, seed in ((11, 600, 3, 12), (1, 500, 5, 13)):
        w = W.any_model(mid, Nx=nx)
        m, _ = orc.model(mid, w["params_true"], w["plength"], w["x"])
        err = 0.002 * np.abs(w["params_true"][w["index_to_relax"]]) + 1e-6
        out.append(dict(mid=mid, w=w, y=synth.make_spectrum(m, seed=seed), nch=nch, err=err, sw=None, pp=None,
                        extra=(0.0, 1.0, 1e30, 0.0), prior=0, seed=seed))
    assert len({f["mid"] for f in out}) == 3 and len({f["nch"] for f in out}) == 3
    assert len({f["w"]["params_true"].size for f in out}) == 3
    return out


def cfg_of(f):
    # the proposal adapts on every iteration, a swap is attempted on every iteration
    return S.default_cfg(f["nch"], seed=f["seed"], Nt_learn=(0, 10 ** 6, 10 ** 6 + 1), periods_learn=(1, 1), prior_fct_switch=f["prior"],
                         dN_mixing=1)


def build(f, orc, lockstep=None):
    ev = None if lockstep is not None else tps.oracle_evaluator(orc, f["mid"], f["w"], f["y"])
    w = f["w"]
    return S.Sampler(cfg_of(f), ev, w["plength"], w["params_true"], w["relax"], f["err"], f["sw"], f["pp"], f["extra"], lockstep=lockstep)


def walk(smp, n_iter, every):
    """init + n_iter iterations in stretches of `every`: (moved, swaps, [state at each checkpoint])."""
    smp.init()
    moved, swaps, marks = [], [], []
    done = 0
    while done < n_iter:
        k = min(every, n_iter - done)
        mv, sw = smp.run(k)
        moved.append(mv); swaps.append(sw)
        marks.append({name: smp.get(name).copy() for name in STATE})
        done += k
    return np.concatenate(moved), np.concatenate(swaps), marks


def same_path(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert len(a[2]) == len(b[2])
    for ma, mb in zip(a[2], b[2]):
        for name in STATE:
            assert np.array_equal(ma[name].view(np.int64), mb[name].view(np.int64)), name


def oracle_backend(orc, members, fail_at=None):
    calls = [0]

    def f(P_list, T_list):
        calls[0] += 1
        if fail_at is not None and calls[0] == fail_at:
            raise RuntimeError("backend failure injected by the test")
        L, st = [], []
        for m, P, T in zip(members, P_list, T_list):
            if P.shape[0] == 0:
                L.append(np.empty(0)); st.append(np.empty(0, dtype=np.int32))
                continue
            l, s = orc.generate_batch(m["mid"], m["w"]["plength"], m["w"]["x"], m["y"], np.ascontiguousarray(P), np.ascontiguousarray(T),
                                      nthreads=1)
            L.append(l); st.append(s)
        return L, st
    f.calls = calls
    return f


def run_together(orc, members, n_iters, every):
    """One thread per member through one lockstep object; every member is joined before the first thread starts and
    leaves when it is done.  Returns the members' walks and the object."""
    ls = S.Lockstep(oracle_backend(orc, members), [m["w"]["params_true"].size for m in members])
    smps = [build(m, orc, lockstep=(ls, k)) for k, m in enumerate(members)]
    for k in range(len(members)):
        ls.join(k)
    out, errs = [None] * len(members), []

    def work(k):
        try:
            out[k] = walk(smps[k], n_iters[k], every)
        except BaseException as e:       # noqa: BLE001
            errs.append(e)
        finally:
            ls.leave(k)
    th = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(len(members))]
    for t in th:
        t.start()
    for t in th:
        t.join(JOIN_TIMEOUT)
    assert not any(t.is_alive() for t in th), "a sampler thread did not end: deadlock in the lockstep object"
    assert not errs and not ls.errors, (errs, ls.errors)
    return out, ls, smps


def test_three_samplers_in_lockstep_walk_their_solo_paths(orc):
    members = fits(orc)
    n = 300
    alone = [walk(build(m, orc), n, 50) for m in members]
    together, ls, smps = run_together(orc, members, [n] * 3, 50)
    for a, b in zip(alone, together):
        same_path(a, b)
    assert alone[0][0].mean() > 0.02 and (alone[0][1] >= 0).sum() == n - 1      # moves happen, swaps are attempted
    # every member was joined before the first thread started: full rounds, one call for the initial evaluation and one per
    # iteration and stretch -- a third of what the three make alone
    assert ls.calls() == n + 1
    for s in smps:
        s.close()
    ls.close()


def test_members_that_run_different_lengths_leave_as_they_finish(orc):
    members = fits(orc)
    n_iters = [50, 120, 200]
    alone = [walk(build(m, orc), n, 50) for m, n in zip(members, n_iters)]
    together, ls, smps = run_together(orc, members, n_iters, 50)
    for a, b in zip(alone, together):
        same_path(a, b)
    assert ls.calls() == max(n_iters) + 1
    for s in smps:
        s.close()
    ls.close()


def test_a_failed_round_reaches_every_member_and_all_can_leave(orc):
    members = fits(orc)
    backend = oracle_backend(orc, members, fail_at=8)       # call 1 is the initial evaluation, so call 8 is the round of iteration 6
    ls = S.Lockstep(backend, [m["w"]["params_true"].size for m in members])
    smps = [build(m, orc, lockstep=(ls, k)) for k, m in enumerate(members)]
    for k in range(3):
        ls.join(k)
    res = [None] * 3

    def work(k):
        try:
            smps[k].init()
            smps[k].run(40)
            res[k] = "finished"
        except capi.AccelError as e:
            res[k] = (e.code, smps[k].iteration())
        finally:
            ls.leave(k)
    th = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join(JOIN_TIMEOUT)
    assert not any(t.is_alive() for t in th)
    assert res == [(capi.E_INVALID, 6)] * 3, res                # the backend's code, in the same iteration for all
    assert backend.calls[0] == 8 and len(ls.errors) == 1
    assert "lockstep backend" in ls.error()
    for s in smps:
        s.close()
    ls.close()                                                  # (destroy succeeds: nobody is joined)


def test_abi_misuse_without_a_device():
    lib = S._lib()
    vp = C.c_void_p
    npar = np.array([4, 7], dtype=np.int32)
    cb = S.GROUP_EVAL_FN(lambda *a: 0)
    h = vp()
    INV = capi.E_INVALID
    assert lib.tamcmc_lockstep_create(None, 2, S._ip(npar), cb, None) == INV
    assert lib.tamcmc_lockstep_create(C.byref(h), 0, S._ip(npar), cb, None) == INV and not h.value
    assert lib.tamcmc_lockstep_create(C.byref(h), 2, None, cb, None) == INV and not h.value
    assert lib.tamcmc_lockstep_create(C.byref(h), 2, S._ip(npar), C.cast(None, S.GROUP_EVAL_FN), None) == INV and not h.value
    assert lib.tamcmc_lockstep_create_group(C.byref(h), None) == INV and not h.value
    assert lib.tamcmc_lockstep_create_group(None, None) == INV
    for fn in (lib.tamcmc_lockstep_join, lib.tamcmc_lockstep_leave, lib.tamcmc_lockstep_collect):
        assert fn(None, 0) == INV
    assert lib.tamcmc_lockstep_destroy(None) == 0               # like the other destroy calls: nothing to do
    assert lib.tamcmc_lockstep_create(C.byref(h), 2, S._ip(npar), cb, None) == 0 and h.value
    for member in (-1, 2, 1 << 20):
        assert lib.tamcmc_lockstep_join(h, member) == INV and lib.tamcmc_lockstep_leave(h, member) == INV
        assert lib.tamcmc_lockstep_collect(h, member) == INV
    assert lib.tamcmc_lockstep_leave(h, 0) == INV               # has not joined
    assert lib.tamcmc_lockstep_join(h, 0) == 0
    assert lib.tamcmc_lockstep_join(h, 0) == INV                # twice
    assert lib.tamcmc_lockstep_destroy(h) == INV                # a member is joined
    P, T, L, st = np.zeros((2, 4)), np.ones(2), np.zeros(2), np.zeros(2, dtype=np.int32)
    dep = lib.tamcmc_lockstep_deposit
    assert dep(h, 1, 2, 7, S._dp(P), S._dp(T), S._dp(L), S._ip(st)) == INV     # member 1 has not joined
    assert dep(h, 0, 2, 5, S._dp(P), S._dp(T), S._dp(L), S._ip(st)) == INV     # not member 0's Nparams
    assert dep(h, 0, 0, 4, S._dp(P), S._dp(T), S._dp(L), S._ip(st)) == INV
    assert dep(h, 0, 2, 4, None, S._dp(T), S._dp(L), S._ip(st)) == INV
    assert lib.tamcmc_lockstep_collect(h, 0) == INV             # nothing deposited
    assert dep(h, 0, 2, 4, S._dp(P), S._dp(T), S._dp(L), S._ip(st)) == 0       # the only joined member: the round fires
    assert dep(h, 0, 2, 4, S._dp(P), S._dp(T), S._dp(L), S._ip(st)) == INV     # a second deposit before collect
    assert lib.tamcmc_lockstep_leave(h, 0) == INV               # inside a round it has deposited into
    assert lib.tamcmc_lockstep_collect(h, 0) == 0
    assert lib.tamcmc_lockstep_calls(h) == 1
    # a sampler for a member that does not exist, or with another fit's parameter count
    w = W.any_model(1, Nx=64)
    cfg = S.default_cfg(3)
    sw, pp, ex = np.zeros(7, dtype=np.int32), np.zeros((4, 7)), np.array([0.0, 1.0, 1e30, 0.0])
    err = np.ones(7)
    common = (7, S._ip(w["plength"]), S._dp(w["params_true"]), S._ip(w["relax"]), S._ip(sw), S._dp(pp), 4, S._dp(ex), S._dp(err))
    sh = vp()
    create = lib.tamcmc_sampler_create_lockstep
    assert create(C.byref(sh), C.byref(cfg), None, 1, *common) == INV and not sh.value
    assert create(C.byref(sh), C.byref(cfg), h, 2, *common) == INV and not sh.value
    assert create(C.byref(sh), C.byref(cfg), h, 0, *common) == INV and not sh.value     # member 0 has 4 parameters
    assert create(C.byref(sh), C.byref(cfg), h, 1, *common) == 0 and sh.value
    assert lib.tamcmc_sampler_init(sh) == INV                   # member 1 has not joined
    lib.tamcmc_sampler_destroy(sh)
    assert lib.tamcmc_lockstep_leave(h, 0) == 0
    assert lib.tamcmc_lockstep_destroy(h) == 0
