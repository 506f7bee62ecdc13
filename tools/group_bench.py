"""Fit groups against one context at a time (developer tool; bench.py stays the headline benchmark).

Per step, four ways, wall clock over --steps steps after --warmup (min / median / max, microseconds):
  solo     the members' eval_batch calls back to back (what a caller without groups does)
  streams  every member's tamcmc_eval_batch_begin first (each context has a stream of its own), then every _end
  group    one tamcmc_group_eval call
  group_begin_end  tamcmc_group_eval_begin + _end (mapped staging, no copies)
for (a) the 8 slices of the reference's local example, 10 chains each, and (b) four synthetic global stars on different
grids (6e4 / 8e4 / 1e5 / 1.2e5 bins), 16 chains each.  Every way computes the same bits; the tool checks that first.
lockstep_sampler: iterations per second of the 8 slices' samplers (10 chains each, a swap attempt per iteration), all of them
through one lockstep object over one group (8 threads) against the same 8 samplers one after the other on
tamcmc_sampler_create_hip, with the proposal adapting on every iteration and with it frozen; the final states must be the
same bits.

    python tools/group_bench.py [--steps 2000] [--warmup 200]
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tamcmc_amd  # noqa: E402
from tamcmc_amd import sampler as S  # noqa: E402
from tamcmc_amd import synth  # noqa: E402
from tamcmc_amd.setup_io import Setup, model_file_slices  # noqa: E402

G = os.path.join(ROOT, "tests", "golden", "ref_inputs")


def slices(nchains):
    model, data, cfg = (os.path.join(G, "TF_3443483_local-v3.model"), os.path.join(G, "TF_3443483_local-v3.data"),
                        os.path.join(G, "Config_default"))
    out = []
    for k in range(len(model_file_slices(model))):
        s = Setup(cfg).load(model, data, k)
        rng = np.random.default_rng(10 + k)
        P = np.tile(s.inputs, (nchains, 1))
        P[1:, s.index_to_relax] += 0.3 * s.err * rng.standard_normal((nchains - 1, s.Nvars))
        acc = tamcmc_amd.Accel(s.model_case, s.plength, s.x, s.y, likelihood_case=s.likelihood_case, likelihood_p=s.likelihood_p)
        out.append((acc, P, 1.7 ** np.arange(nchains), s))
    return out


def stars(nchains, sizes=(60000, 80000, 100000, 120000)):
    out = []
    for j, nx in enumerate(sizes):
        w = synth.workload_c2(Nx=nx)
        with tamcmc_amd.Accel(2, w["plength"], w["x"], np.ones(nx)) as a0:
            m, st = a0.model_explicit(w["params_true"])
        acc = tamcmc_amd.Accel(2, w["plength"], w["x"], synth.make_spectrum(m, seed=100 + j))
        out.append((acc, synth.chain_params(w, nchains, seed=j + 1), synth.temperatures(nchains)))
    return out


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t = np.empty(steps)
    for i in range(steps):
        t0 = time.perf_counter()
        fn()
        t[i] = time.perf_counter() - t0
    return dict(min_us=round(1e6 * float(t.min()), 2), median_us=round(1e6 * float(np.median(t)), 2),
                max_us=round(1e6 * float(t.max()), 2))


def compare(members, steps, warmup):
    accs = [m[0] for m in members]
    P_list, T_list = [m[1] for m in members], [m[2] for m in members]
    with tamcmc_amd.Group(accs) as g:
        L, st = g.eval(P_list, T_list)
        for a, P, T, l in zip(accs, P_list, T_list, L):
            assert np.array_equal(a.eval_batch(P, T)[0].view(np.int64), l.view(np.int64))
        g.begin(P_list, T_list)
        for l, l2 in zip(L, g.end()[0]):
            assert np.array_equal(l.view(np.int64), l2.view(np.int64))

        def solo():
            for a, P, T in zip(accs, P_list, T_list):
                a.eval_batch(P, T)

        def streams():
            for a, P, T in zip(accs, P_list, T_list):
                a.begin(P, T)
            for a in accs:
                a.end()

        def halves():
            g.begin(P_list, T_list)
            g.end()

        res = {"solo": timed(solo, steps, warmup), "streams": timed(streams, steps, warmup),
               "group": timed(lambda: g.eval(P_list, T_list), steps, warmup), "group_begin_end": timed(halves, steps, warmup)}
    res["group_vs_solo"] = round(res["solo"]["median_us"] / res["group"]["median_us"], 2)
    res["group_begin_end_vs_group"] = round(res["group"]["median_us"] / res["group_begin_end"]["median_us"], 2)
    res["group_begin_end_vs_streams"] = round(res["streams"]["median_us"] / res["group_begin_end"]["median_us"], 2)
    return res


def lockstep_sampler(members, n_iter):
    """Wall time of n_iter iterations of every slice's sampler: one after the other (create_hip), and together."""
    accs = [m[0] for m in members]
    sets = [m[3] for m in members]
    nch = members[0][1].shape[0]
    out = {"iterations": n_iter, "slices": len(members), "chains": nch}
    for mode, learn in (("adapting", (0, 10 ** 9, 10 ** 9 + 1)), ("frozen", (10 ** 9, 10 ** 9 + 1, 10 ** 9 + 2))):
        def make(k, **kw):
            s = sets[k]
            cfg = s.sampler_cfg(seed=42)
            cfg.Nchains = cfg.Nchains_local = nch
            cfg.lambda_temp, cfg.dN_mixing, cfg.n_learn = 1.7, 1, 3
            for i, v in enumerate(learn):
                cfg.Nt_learn[i] = v
            cfg.periods_learn[0] = cfg.periods_learn[1] = 1
            return S.Sampler(cfg, kw.get("acc"), s.plength, s.inputs, s.relax, s.err, s.priors_names_switch, s.priors, s.extra_priors,
                             lockstep=kw.get("lockstep"))
        solo = [make(k, acc=accs[k]) for k in range(len(accs))]
        for smp in solo:
            smp.init()
            smp.run(200, history=False)                 # warm-up
        t0 = time.perf_counter()
        for smp in solo:
            smp.run(n_iter, history=False)
        t_seq = time.perf_counter() - t0
        with tamcmc_amd.Group(accs) as g:
            ls = S.Lockstep(g)
            tog = [make(k, lockstep=(ls, k)) for k in range(len(accs))]
            for k in range(len(accs)):
                ls.join(k)
            gate = threading.Barrier(len(accs) + 1)
            errs = []

            def work(k):
                try:
                    tog[k].init()
                    tog[k].run(200, history=False)
                    gate.wait(300)
                    tog[k].run(n_iter, history=False)
                except BaseException as e:      # noqa: BLE001
                    errs.append(e)
                    gate.abort()
                finally:
                    ls.leave(k)
            th = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(len(accs))]
            for t in th:
                t.start()
            gate.wait(300)
            t0 = time.perf_counter()
            for t in th:
                t.join(600)
            t_tog = time.perf_counter() - t0
            if errs or any(t.is_alive() for t in th):
                raise RuntimeError(f"lockstep run failed: {errs} {ls.error()}")
            for a, b in zip(solo, tog):
                for name in ("vars", "logL", "sigma", "covarmat"):
                    assert np.array_equal(a.get(name).view(np.int64), b.get(name).view(np.int64)), name
            calls = ls.calls()
            for smp in tog:
                smp.close()
            ls.close()
        for smp in solo:
            smp.close()
        out[mode] = {"sequential_s": round(t_seq, 4), "together_s": round(t_tog, 4),
                     "sequential_it_per_s": round(n_iter / t_seq, 1), "together_it_per_s": round(n_iter / t_tog, 1),
                     "speedup": round(t_seq / t_tog, 2), "group_calls": calls}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--sampler-iterations", type=int, default=3000)
    args = ap.parse_args()
    out = {"version": tamcmc_amd.capi.version()}
    m = slices(10)
    out["local_8_slices_x_10_chains"] = compare(m, args.steps, args.warmup)
    out["lockstep_sampler"] = lockstep_sampler(m, args.sampler_iterations)
    for a in m:
        a[0].close()
    m = stars(16)
    out["4_stars_x_16_chains"] = compare(m, max(args.steps // 4, 10), max(args.warmup // 4, 5))
    for a, _, _ in m:
        a.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
