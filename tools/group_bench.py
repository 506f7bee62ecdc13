"""Fit groups against one context at a time (developer tool; bench.py stays the headline benchmark).

Per step, three ways, wall clock over --steps steps after --warmup (min / median / max, microseconds):
  solo     the members' eval_batch calls back to back (what a caller without groups does)
  streams  every member's tamcmc_eval_batch_begin first (each context has a stream of its own), then every _end
  group    one tamcmc_group_eval call
for (a) the 8 slices of the reference's local example, 10 chains each, and (b) four synthetic global stars on different
grids (6e4 / 8e4 / 1e5 / 1.2e5 bins), 16 chains each.  Every way computes the same bits; the tool checks that first.

    python tools/group_bench.py [--steps 2000] [--warmup 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tamcmc_amd  # noqa: E402
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
        out.append((acc, P, 1.7 ** np.arange(nchains)))
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

        def solo():
            for a, P, T in zip(accs, P_list, T_list):
                a.eval_batch(P, T)

        def streams():
            for a, P, T in zip(accs, P_list, T_list):
                a.begin(P, T)
            for a in accs:
                a.end()

        res = {"solo": timed(solo, steps, warmup), "streams": timed(streams, steps, warmup),
               "group": timed(lambda: g.eval(P_list, T_list), steps, warmup)}
    res["group_vs_solo"] = round(res["solo"]["median_us"] / res["group"]["median_us"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    args = ap.parse_args()
    out = {"version": tamcmc_amd.capi.version()}
    m = slices(10)
    out["local_8_slices_x_10_chains"] = compare(m, args.steps, args.warmup)
    for a, _, _ in m:
        a.close()
    m = stars(16)
    out["4_stars_x_16_chains"] = compare(m, max(args.steps // 4, 10), max(args.warmup // 4, 5))
    for a, _, _ in m:
        a.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
