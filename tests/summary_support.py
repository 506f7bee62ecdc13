"""What two or more of the posterior-summary suites use (tests/test_summary_*_gpu.py, tests/test_cli_*_gpu.py,
tests/test_scan_null_gpu.py, tests/test_summary_*_host.py): the cases and their references, the bit-for-bit comparisons, the
common body of the three tail checks, the accumulation-alone reference of the fold, the PSIS-LOO reference with its check and
the exact cutoff from the library's own l, the ESS and band-ESS passes with the checks of the lag products and the finish, and the stored chain of the command-line tests.
Importing this module needs no GPU.

Tolerances of reference() / check() are derived, not tuned: the project's per-bin model bar eps = 1e-12 (RTOL_MODEL,
tests/test_parity_gpu.py) propagated through each statistic, plus n 2^-52 (relative) for the accumulation over n samples,
E = eps + n 2^-52:
    |d mean_M| <= E mean|M|          |d var_M| <= 4 E mean(M^2)          min_M, max_M: eps relative
    chi(2,2p)    |d l| <= p eps (y/M + 1)                      }  =: delta_i, the maximum over the samples,
    chi_square   |d l| <= (2 |y - M| eps M + (eps M)^2) / s^2  }     plus n 2^-52 max|l|
    |d mean_l|, |d lppd| <= delta_i          |d var_l| <= 2 delta_i sqrt(var_l) + delta_i^2
    totals: the sum of the per-bin bounds (waic: twice the sum of the lppd and var_l bounds)
"""
import functools
import math
import os
import re

import numpy as np

import ess_reference as R
import workloads as W
from support import CFG, DATA, LD, MODEL, ROOT, bits, pyorc, tool
from tamcmc_amd import capi, synth

EPS = 1e-12
ULP = 2.0 ** -52
ARRAYS = capi.Summary.ARRAYS
TOTALS = ("n_used", "n_rejected", "lppd_total", "p_waic", "waic")


# ---- cases and data ----

def spectrum_for(w, seed=17):
    m, st = pyorc().model(w["model_case"], w["params_true"], w["plength"], w["x"])
    assert st == 0, (w["model_case"], st)
    return synth.make_spectrum(m, seed=seed)


def true_model(w):
    m, st = pyorc().model(w["model_case"], w["params_true"], w["plength"], w["x"])
    assert st == 0, (w["model_case"], st)
    return m


def sigma_of(n):
    return 0.05 + 0.2 * np.abs(np.sin(np.arange(n)))        # (tests/test_parity_gpu.py::test_chi_square_likelihood)


def reference(w, y, P, sigma=None, like=0, p=1.0):
    """Long-double reduction of the oracle's rows of the accepted samples, and the bounds of the module docstring."""
    mid = w["model_case"]
    rL, rst, M = pyorc().generate_batch(mid, w["plength"], w["x"], y, P, np.ones(len(P)), sigma_y=sigma, likelihood_case=like,
                                        likelihood_p=p, want_models=True)
    ok = rst == 0
    n = int(ok.sum())
    Mq, yq = M[ok].astype(LD), y.astype(LD)
    pt = float(int(p))                                  # `long p`, likelihoods.cpp:17
    if like == 0:
        l = -pt * (yq / Mq + np.log(Mq))
        dl = pt * EPS * (yq / Mq + 1.0)
    else:
        s2 = sigma.astype(LD) ** 2
        l = -((yq - Mq) ** 2) / s2
        dl = (2.0 * np.abs(yq - Mq) * EPS * Mq + (EPS * Mq) ** 2) / s2
    ref = dict(n_used=n, n_rejected=int((~ok).sum()), status=rst, logL=rL)
    if n == 0:
        return ref, {}
    acc = n * 2.0 ** -52
    E = EPS + acc
    mean_M, mean_l = Mq.mean(axis=0), l.mean(axis=0)
    a = l.max(axis=0)
    ref.update(mean_M=mean_M, min_M=Mq.min(axis=0), max_M=Mq.max(axis=0), mean_l=mean_l,
               lppd=a + np.log(np.exp(l - a).sum(axis=0) / n))
    delta = dl.max(axis=0) + acc * np.abs(l).max(axis=0)
    bound = dict(mean_M=E * np.abs(Mq).mean(axis=0), min_M=EPS * np.abs(ref["min_M"]), max_M=EPS * np.abs(ref["max_M"]),
                 mean_l=delta, lppd=delta)
    ref["lppd_total"] = ref["lppd"].sum()
    bound["lppd_total"] = delta.sum()
    if n >= 2:
        ref["var_M"] = ((Mq - mean_M) ** 2).sum(axis=0) / (n - 1)
        ref["var_l"] = ((l - mean_l) ** 2).sum(axis=0) / (n - 1)
        bound["var_M"] = 4.0 * E * (Mq ** 2).mean(axis=0)
        bound["var_l"] = 2.0 * delta * np.sqrt(ref["var_l"]) + delta ** 2
        ref["p_waic"] = ref["var_l"].sum()
        bound["p_waic"] = bound["var_l"].sum()
        ref["waic"] = -2.0 * (ref["lppd_total"] - ref["p_waic"])
        bound["waic"] = 2.0 * (bound["lppd_total"] + bound["p_waic"])
    return ref, bound


def check(tag, res, ref, bound):
    """Every array and total of `res` within its bound; prints the worst ratio of each first."""
    assert res["n_used"] == ref["n_used"] and res["n_rejected"] == ref["n_rejected"], (tag, res["n_used"], res["n_rejected"])
    worst = {}
    for k, b in bound.items():
        err = np.abs(np.asarray(res[k], dtype=LD) - ref[k])
        assert np.all(np.isfinite(np.asarray(res[k]))), (tag, k)
        worst[k] = float(np.max(err / b)) if np.all(np.asarray(b) > 0) else (0.0 if np.all(err == 0) else np.inf)
    print(f"RATIO {tag}: " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (tag, k, v)
    if ref["n_used"] < 2:
        assert np.all(np.isnan(res["var_M"])) and np.all(np.isnan(res["var_l"])) and np.isnan(res["p_waic"]) and np.isnan(res["waic"]), \
            (tag, "var_M, var_l, p_waic, waic of fewer than two samples")
    return worst


def summarize(acc, pushes, block_chains=0):
    with capi.Summary(acc, block_chains) as s:
        out = [s.push(P) for P in pushes]
        return s.result(), np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


@functools.lru_cache(maxsize=None)
def c2_case(Nx, S=37):
    """Id 2 on the C2 star's grid: workload, spectrum, S chain rows and the reference (computed once, never changed)."""
    w = synth.workload_c2(Nx=Nx)
    y = spectrum_for(w)
    P = synth.chain_params(w, S)
    ref, bound = reference(w, y, P)
    for a in (y, P):
        a.setflags(write=False)
    return w, y, P, ref, bound


@functools.lru_cache(maxsize=None)
def c2_chain(Nx, S, scale=0.5):
    """Id 2 on the C2 star's grid without a reference: workload, spectrum, S chain rows (computed once, never changed)."""
    w = synth.workload_c2(Nx=Nx)
    y = spectrum_for(w)
    P = synth.chain_params(w, S, scale=scale)
    for a in (y, P):
        a.setflags(write=False)
    return w, y, P


def rows_around(w, n, seed=20261, scale=0.5):
    """As chains_around (tests/test_group_gpu.py): row 0 is the truth, the others the truth + scale err normal."""
    rng = np.random.default_rng(seed)
    idx = w["index_to_relax"]
    P = np.tile(w["params_true"], (n, 1))
    P[1:, idx] += scale * w["err"][None, :] * rng.standard_normal((n - 1, idx.size))
    return P


def other_cases():
    c1 = synth.workload_c1(Nx=1000)
    return {
        "c1-id11-fused": (c1, synth.chain_params(c1, 37), {}),
        "id14": (W.any_model(14, Nx=3000), None, {}),
        "id3-asym10": (synth.workload_c2(model_case=3, Nx=3000, asym=10.0), None, {}),
        "p=2": (W.make(2, Nx=3000), None, dict(p=2.0)),
        "chi-square-id0": (W.any_model(0, Nx=3000), None, dict(like=1, sigma=sigma_of(3000))),
        "chi-square-id2": (W.any_model(2, Nx=3000), None, dict(like=1, sigma=sigma_of(3000))),
    }


def gpu_rows(acc, P):
    """(logL, status, model rows) of every row of P from the GPU."""
    return acc.eval_batch(P, np.ones(len(P)), model_rows=np.arange(len(P)))


def row_groups(P):
    """Index of each row's first identical row: duplicated parameter rows share their perturbation."""
    _, inv = np.unique(np.ascontiguousarray(P), axis=0, return_inverse=True)
    return np.asarray(inv).reshape(-1)


def perturbed_rows(rows, rel, seed, groups):
    """rows (1 + rel s), s = +-1, one sign per distinct parameter row and bin."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2, size=(int(groups.max()) + 1, rows.shape[1])) * 2 - 1
    r = np.asarray(rows).astype(LD)
    return r * (1 + LD(rel) * s[groups].astype(LD))


def diff(key, a, b):
    """max over the bins of the difference of two results of `key`: relative to max(1, |b|), absolute for pit; where a
    value is infinite both must be the same infinity (else inf)."""
    a, b = np.asarray(a).astype(LD), np.asarray(b).astype(LD)
    fin = np.isfinite(a) & np.isfinite(b)
    if not np.array_equal(a[~fin], b[~fin]):
        return np.inf
    if not fin.any():
        return 0.0
    d = np.abs(a[fin] - b[fin])
    if key != "pit":
        d = d / np.maximum(1, np.abs(b[fin]))
    return float(np.max(d))


def edited(y, like=0, M0=None, sigma=None):
    """The data edits of a case, on a copy: (y, dict name -> bin).  chi(2,2p): one y times 2000 (the largest datum, so that
    y / M is not small to begin with), one 0, one 1e-300, one negative; chi_square: y at M0 + 40 sigma and at M0 - 40 sigma,
    M0 the model at the chain's centre."""
    y = np.array(y)
    nx = y.size
    where = {}
    if like == 0:
        if nx < 8:
            where = dict(zero=nx - 1)
        else:
            top = int(np.argmax(y))
            free = [k for k in range(3, nx, 14) if k != top]
            where = dict(x2000=top, zero=free[0], tiny=free[1], negative=free[2])
        for name, k in where.items():
            y[k] = dict(x2000=2000.0 * y[k], zero=0.0, tiny=1e-300, negative=-abs(y[k]) - 1.0)[name]
    elif nx >= 8:
        where = dict(plus40=5, minus40=nx - 3)
        y[5] = M0[5] + 40.0 * sigma[5]
        y[nx - 3] = M0[nx - 3] - 40.0 * sigma[nx - 3]
    return y, where


def edited_chi(y):
    """The chi(2,2p) data edits, on a copy: three neighbouring bins -- inside one window wherever W >= 7 -- hold a datum
    times 2000, a 0 and a negative one; a grid shorter than 7 bins gets the 0 alone."""
    y = np.array(y)
    if y.size < 7:
        y[-1] = 0.0
    else:
        y[4] *= 2000.0
        y[5] = 0.0
        y[6] = -abs(y[6]) - 1.0
    return y


def with_rejected(w, P, at):
    """P with a row whose first relaxed parameter is NaN inserted before each position of `at`."""
    bad = np.array(P[0])
    bad[w["index_to_relax"][0]] = np.nan
    return np.insert(np.array(P), at, bad, axis=0)


def accepted(acc, P, n_bad):
    _, st, rows = gpu_rows(acc, P)
    assert int((st != 0).sum()) == n_bad, ("rejected samples", int((st != 0).sum()), n_bad)
    return rows[st == 0]


def open_case(accel_mod, w, y, cfg):
    if cfg == "chi-square":
        return accel_mod.Accel(2, w["plength"], w["x"], y, sigma_y=sigma_of(len(y)), likelihood_case=1)
    return accel_mod.Accel(2, w["plength"], w["x"], y, likelihood_p=float(cfg[1:]) + 0.5)      # truncated as everywhere


def data_of(w, y0, cfg):
    """(y, like, p, sigma) of a likelihood configuration "p1", "p3", ... or "chi-square"."""
    if cfg == "chi-square":
        sigma = sigma_of(len(y0))
        y = edited(y0, 1, true_model(w), sigma)[0]
        return y, 1, 1, sigma
    return edited_chi(y0), 0, int(cfg[1:]), None


# ---- two results bit for bit ----

def same(r1, r2):
    """Two fold results bit for bit: every array and every total (NaN == NaN when the bits agree)."""
    return all(np.array_equal(bits(r1[k]), bits(r2[k])) for k in ARRAYS) and \
        all(np.array_equal(bits(float(r1[k])), bits(float(r2[k]))) for k in TOTALS)


def same_pred(r1, r2):
    return all(np.array_equal(bits(r1[k]), bits(r2[k])) for k in capi.Summary.PREDICTIVE_ARRAYS) and \
        np.array_equal(r1["pit_hist"], r2["pit_hist"]) and \
        all(np.array_equal(bits(float(r1[k])), bits(float(r2[k]))) for k in capi.Summary.PREDICTIVE_TOTALS)


def same_win(r1, r2):
    return all(np.array_equal(bits(r1[k]), bits(r2[k])) for k in capi.Summary.WINDOW_ARRAYS) and \
        np.array_equal(r1["pit_hist"], r2["pit_hist"]) and \
        all(np.array_equal(bits(float(r1[k])), bits(float(r2[k]))) for k in capi.Summary.WINDOW_TOTALS) and \
        np.array_equal(r1["first_bin"], r2["first_bin"]) and np.array_equal(r1["last_bin"], r2["last_bin"])


def same_scan(r1, r2):
    return all(np.array_equal(bits(r1[k]), bits(r2[k])) for k in capi.Summary.SCAN_ARRAYS) and \
        all(np.array_equal(bits(float(r1[k])), bits(float(r2[k]))) for k in capi.Summary.SCAN_TOTALS) and \
        np.array_equal(r1["first_bin"], r2["first_bin"]) and np.array_equal(r1["last_bin"], r2["last_bin"])


def same_scans(a, b):
    return len(a) == len(b) and all(same_scan(x, y) for x, y in zip(a, b))


# ---- quantiles: the truth and the selection loop ----

Q8 = (0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0, 0.5)        # the last one is a duplicate
ONE = np.uint64(1)


def ranks_of(q, n):
    return np.array([min(max(int(math.ceil(t * float(n))) - 1, 0), n - 1) for t in q])


def truth_of(rows, q):
    """(Nq, Nx): the order statistics of the accepted rows."""
    return np.sort(rows, axis=0)[ranks_of(q, len(rows))]


def keys(a):
    u = (np.asarray(a, dtype=np.float64) + 0.0).view(np.uint64)
    return np.where((u >> np.uint64(63)) != 0, ~u, u | (ONE << np.uint64(63)))


def unresolved_bits(rows):
    """max over the bins of bit_length(key(max) - key(min))."""
    k = keys(rows)
    return max(int(r).bit_length() for r in (k.max(axis=0) - k.min(axis=0)))


def select(s, q, nbits, push_pass, truth=None, u0=None):
    """begin, then passes of push_pass(pass number) + step until 0 bits are left.  Returns the brackets after begin and after
    every step.  With `truth`: containment and monotony after every step; with `u0`: bits_left after every step."""
    b = nbits if nbits else 6
    s.quantiles_begin(q, nbits)
    r = s.quantiles_result()
    traj = [(r["lo"], r["hi"])]
    left, steps = None, 0
    while left != 0:
        push_pass(steps)
        left = s.quantiles_step()
        steps += 1
        assert steps <= -(-64 // b), "more steps than ceil(64 / bits)"
        r = s.quantiles_result()
        if u0 is not None:
            assert left == max(u0 - steps * b, 0), (steps, left, u0)
        elif len(traj) > 1:
            assert left == max(prev_left - b, 0), (steps, left, prev_left)
        prev_left = left
        if truth is not None:
            assert np.all(r["lo"] <= truth) and np.all(truth <= r["hi"]), f"step {steps}: the bracket lost the truth"
        assert np.all(r["lo"] >= traj[-1][0]) and np.all(r["hi"] <= traj[-1][1]), f"step {steps}: a bracket grew"
        traj.append((r["lo"], r["hi"]))
    return traj, r["ranks"]


def steps(s, q, nbits, push_pass, truth, limit):
    """select(), ended after `limit` steps: the trajectory so far."""
    s.quantiles_begin(q, nbits)
    r = s.quantiles_result()
    traj = [(r["lo"], r["hi"])]
    for k in range(limit):
        push_pass(k)
        s.quantiles_step()
        r = s.quantiles_result()
        assert np.all(r["lo"] <= truth) and np.all(truth <= r["hi"]), f"step {k + 1}: the bracket lost the truth"
        traj.append((r["lo"], r["hi"]))
    s.quantiles_end()
    return traj


def same_traj(t1, t2):
    return len(t1) == len(t2) and all(np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) for a, b in zip(t1, t2))


# ---- the tail checks (per bin, per window, per scan position) against their references ----

def check_tails_reference(reference, label, keys, tag, res, rows, y, groups, rel, seeds, with_f64, like, shape, f64_always,
                          positions=None, worst=None):
    """Common body of the predictive, window and scan suites' check_reference.  `reference(rows, y[, dtype=])` is the
    suite's long-double reference with its case bound in; `res` is checked against reference(rows, y) on `keys` (at
    `positions` of res, where given) within 10 x the larger of
        (a) the reference's own change under a `rel` relative perturbation of the rows, the maximum over `seeds`, and
        (b) with `with_f64`, its float64-minus-long-double difference.
    Then the self-check |exp(log_cdf) + exp(log_sf) - 1| <= (n + 2) 2^-52, plus 10 x (b) where the shape `shape` of a
    chi(2,2p) tail exceeds 1.  The float64 run is made under `with_f64`, or always with `f64_always`: without it (b) is 0
    in the self-check's slack too.  Prints `RATIO <label> <tag>:` and `SELF <label> <tag>:` before it asserts; `worst`, a
    dict, collects the worst ratio per key under the tag's first word.  Returns the reference."""
    n = len(rows)
    sel = slice(None) if positions is None else np.asarray(positions)
    ref = reference(rows, y)
    d = {k: 0.0 for k in keys}
    for seed in seeds:
        pert = reference(perturbed_rows(rows, rel, seed, groups), y)
        for k in keys:
            d[k] = max(d[k], diff(k, pert[k], ref[k]))
    b64 = {k: 0.0 for k in keys}
    if with_f64 or f64_always:
        r64 = reference(rows, y, dtype=np.float64)
        b64 = {k: diff(k, r64[k], ref[k]) for k in keys}         # bound (b): part of the bound on the GPU's own rows, and of the self-check's slack
    if with_f64:
        for k in keys:
            d[k] = max(d[k], b64[k])
    for k, dk in d.items():
        assert np.isfinite(dk), (tag, k, "the reference runs disagree on where the value is finite: the case has no bound")
    ratios = {}
    for k, dk in d.items():
        err = diff(k, np.asarray(res[k])[sel], ref[k])
        ratios[k] = err / (10.0 * dk) if dk > 0 else (0.0 if err == 0 else np.inf)
    print(f"RATIO {label} {tag}: " + " ".join(f"{k}={v:.3g} (bound {10.0 * d[k]:.3g})" for k, v in ratios.items()))
    seen = {k: 0.0 for k in keys} if worst is None else worst.setdefault(tag.split(" ")[0], {k: 0.0 for k in keys})
    for k, v in ratios.items():
        seen[k] = max(seen[k], v)
        assert v <= 1.0, (tag, k, v)
    # self-check: the two tails sum to 1
    lc, ls = np.asarray(res["log_cdf"]), np.asarray(res["log_sf"])
    one = np.abs(np.exp(lc) + np.exp(ls) - 1.0)[sel]
    slack = (n + 2) * ULP + (10.0 * max(b64["log_cdf"], b64["log_sf"]) if like == 0 and shape > 1 else 0.0)
    print(f"SELF {label} {tag}: |P + Q - 1| = {float(one.max()):.3g} (bound {slack:.3g})")
    assert np.all(one <= slack), (tag, float(one.max()), slack)
    return ref


def check_pit(tag, res):
    """pit from the smaller tail, within 2 ulp; everything in range.  Returns (log_cdf, log_sf, pit) as arrays."""
    lc, ls, pit = np.asarray(res["log_cdf"]), np.asarray(res["log_sf"]), np.asarray(res["pit"])
    want = np.where(lc < ls, np.exp(lc), -np.expm1(ls))      # (the host's exp / expm1 and numpy's: each within an ulp of the truth)
    assert np.all(np.abs(pit - want) <= 2.0 * np.spacing(want)), (tag, "pit")
    assert np.all((pit >= 0) & (pit <= 1)) and np.all(lc <= 0) and np.all(ls <= 0), tag
    return lc, ls, pit


def collect(check, misses, tag, *a, **k):
    """check(tag, ...) with a miss recorded, not raised: every combination of a case is checked and printed before the case
    fails on `assert not misses`."""
    try:
        check(tag, *a, **k)
    except AssertionError as e:
        misses.append(str(e).split("\n")[0])


# ---- the fold: accumulation alone (bound b of tests/test_summary_large_gpu.py) ----

def accumulation_reference(M, y, sigma, like, p=1.0):
    """reference() of tests/summary_support.py on given rows with EPS = 0, plus the rounding of l (module docstring)."""
    n = len(M)
    Mq, yq = M.astype(LD), y.astype(LD)
    if like == 0:
        l = -p * (yq / Mq + np.log(Mq))
        dl = 2.0 * ULP * p * (yq / Mq + np.abs(np.log(Mq)))
    else:
        l = -((yq - Mq) ** 2) / sigma.astype(LD) ** 2
        dl = 3.0 * ULP * np.abs(l)
    acc = n * ULP
    mean_M, mean_l = Mq.mean(axis=0), l.mean(axis=0)
    a = l.max(axis=0)
    ref = dict(n_used=n, n_rejected=0, mean_M=mean_M, min_M=Mq.min(axis=0), max_M=Mq.max(axis=0), mean_l=mean_l,
               lppd=a + np.log(np.exp(l - a).sum(axis=0) / n))
    delta = dl.max(axis=0) + acc * np.abs(l).max(axis=0)
    ref["var_M"] = ((Mq - mean_M) ** 2).sum(axis=0) / (n - 1)
    ref["var_l"] = ((l - mean_l) ** 2).sum(axis=0) / (n - 1)
    bound = dict(mean_M=acc * np.abs(Mq).mean(axis=0), mean_l=delta, lppd=delta, var_M=4.0 * acc * (Mq ** 2).mean(axis=0),
                 var_l=2.0 * delta * np.sqrt(ref["var_l"]) + delta ** 2)
    ref["lppd_total"], bound["lppd_total"] = ref["lppd"].sum(), delta.sum()
    ref["p_waic"], bound["p_waic"] = ref["var_l"].sum(), bound["var_l"].sum()
    ref["waic"], bound["waic"] = -2.0 * (ref["lppd_total"] - ref["p_waic"]), 2.0 * (bound["lppd_total"] + bound["p_waic"])
    return ref, bound


# ---- PSIS-LOO: the reference and its bounds (tests/test_summary_loo_gpu.py has the rule) ----

def tail_M(n):
    return int(math.ceil(min(n / 5.0, 3.0 * math.sqrt(float(n)))))


def psis_reference(x, dtype=LD):
    """The definition, per bin.  x: (n, Nx) values of -l.  Returns elpd_loo, pareto_k, cutoff (dtype) and tail_len."""
    x = np.asarray(x, dtype=dtype)
    n, nx = x.shape
    M = tail_M(n)
    log_min = np.log(dtype(np.finfo(np.float64).tiny))
    eps10 = dtype(10.0 * 2.0 ** -52)
    elpd, khat, cutoff = np.empty(nx, dtype=dtype), np.full(nx, np.inf, dtype=dtype), np.full(nx, np.nan, dtype=dtype)
    tail_len = np.zeros(nx, dtype=np.int32)
    for i in range(nx):
        xs = np.sort(x[:, i])
        xmax = xs[-1]
        z = xs - xmax
        if n > M:
            cutoff[i] = xs[n - M - 1]
            c = max(z[n - M - 1], log_min)
            in_tail = z > c
        else:
            c = dtype(np.inf)
            in_tail = np.zeros(n, dtype=bool)
        tail, body = z[in_tail], z[~in_tail]
        L = tail.size
        tail_len[i] = L
        zt = tail.copy()
        if L >= 5:
            ec = np.exp(c)
            t = np.exp(tail) - ec
            m = 30 + int(math.floor(math.sqrt(L)))
            q = int(math.floor(L / 4.0 + 0.5))
            j = np.arange(1, m + 1).astype(dtype)
            theta = (1 - np.sqrt(dtype(m) / (j - dtype(0.5)))) / (3 * t[q - 1]) + 1 / t[L - 1]
            k = np.array([np.mean(np.log1p(-th * t)) for th in theta], dtype=dtype)
            ell = L * (np.log(-theta / k) - k - 1)
            w = np.array([1 / np.sum(np.exp(ell - lj)) for lj in ell], dtype=dtype)
            w = np.where(w < eps10, dtype(0), w)
            w = w / np.sum(w)
            that = np.sum(w * theta)
            kk = np.mean(np.log1p(-that * t))
            sigma = -kk / that
            kh = (L * kk + 5) / (L + 10)
            khat[i] = kh
            if np.isfinite(kh):
                lp = np.log1p(-(np.arange(1, L + 1).astype(dtype) - dtype(0.5)) / L)
                inner = -sigma * lp if kh == 0 else sigma / kh * np.expm1(-kh * lp)
                zt = np.minimum(np.log(inner + ec), dtype(0))
        elpd[i] = np.log(dtype(body.size) + np.sum(np.exp(zt - tail))) - xmax - np.log(np.sum(np.exp(body)) + np.sum(np.exp(zt)))
    return dict(elpd_loo=elpd, pareto_k=khat, cutoff=cutoff, tail_len=tail_len)


def x_of(rows, y, like=0, p=1.0, sigma=None, dtype=LD):
    """-l of every accepted sample and bin from model rows, in the reference's own arithmetic."""
    Mq, yq = np.asarray(rows).astype(dtype), np.asarray(y).astype(dtype)
    if like == 0:
        return dtype(float(int(p))) * (yq / Mq + np.log(Mq))                 # `long p`, likelihoods.cpp:17
    return ((yq - Mq) ** 2) / np.asarray(sigma).astype(dtype) ** 2          # the reference's convention: no factor 1/2


def perturbed(x, rel, seed, groups):
    """x (1 + rel s), s = +-1, one sign per distinct row and bin."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2, size=(int(groups.max()) + 1, x.shape[1])) * 2 - 1
    return x * (1 + x.dtype.type(rel) * s[groups].astype(x.dtype))


def change(a, b):
    """max over the bins of |a - b| where both are finite; where either is not, both must agree."""
    fa, fb = np.isfinite(a), np.isfinite(b)
    if not np.array_equal(fa, fb):
        return np.inf
    return float(np.max(np.abs(a[fa].astype(LD) - b[fa].astype(LD)))) if fa.any() else 0.0


def check_loo_reference(tag, res, x_ld, groups, rel, seeds, x64=None, totals=True):
    """res against psis_reference(x_ld) with the bounds of the module docstring.  Returns the reference."""
    ref = psis_reference(x_ld)
    d = dict(elpd_loo=0.0, pareto_k=0.0)
    for seed in seeds:
        pert = psis_reference(perturbed(x_ld, rel, seed, groups))
        for k in d:
            d[k] = max(d[k], change(pert[k], ref[k]))
    if x64 is not None:
        r64 = psis_reference(x64, np.float64)
        for k in d:
            d[k] = max(d[k], change(r64[k], ref[k]))
    for k, dk in d.items():                                                  # change() gives inf when two reference runs disagree
        assert np.isfinite(dk), (tag, k, "the reference runs disagree on where the value is finite: the case has no bound")
    assert np.array_equal(res["tail_len"], ref["tail_len"]), (tag, "tail_len")
    assert np.array_equal(np.isinf(res["pareto_k"]), np.isinf(ref["pareto_k"])), (tag, "where k-hat is +inf")
    ratios = {}
    for k, dk in d.items():
        err = change(np.asarray(res[k]), ref[k])
        ratios[k] = err / (10.0 * dk) if dk > 0 else (0.0 if err == 0 else np.inf)
    print(f"RATIO loo {tag}: " + " ".join(f"{k}={v:.3g} (bound {10.0 * d[k]:.3g})" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (tag, k, v)
    if not totals:
        return ref
    # totals: the sums of what was just checked, in long double
    e = np.asarray(res["elpd_loo"]).astype(LD).sum()
    assert res["elpd_loo_total"] == float(e) and res["looic"] == float(-2 * e), tag
    kh = np.asarray(res["pareto_k"])
    assert res["n_k_high"] == int((kh > 0.7).sum()) and res["n_k_inf"] == int(np.isposinf(kh).sum()), tag
    assert res["k_max"] == np.nanmax(kh), tag
    return ref


def library_l(acc, P):
    """l_is bit for bit from the library: after a reset and one sample, mean_l is l."""
    out = np.empty((len(P), acc.Nx))
    with capi.Summary(acc, 1) as s:
        for k in range(len(P)):
            s.reset()
            _, st = s.push(P[k:k + 1])
            assert st[0] == 0
            out[k] = s.result()["mean_l"]
    return out


def exact_structure(tag, res, l):
    """cutoff and tail_len from the library's own l (n, Nx), no tolerance."""
    n = len(l)
    M = tail_M(n)
    xs = np.sort(-l, axis=0)
    assert res["n_used"] == n
    if n <= M:
        assert np.all(np.isnan(res["cutoff"])) and np.all(res["tail_len"] == 0), tag
        return
    cut = xs[n - M - 1]
    assert np.array_equal(bits(res["cutoff"] + 0.0), bits(cut + 0.0)), (tag, "cutoff")
    z = xs - xs[-1]
    c = np.maximum(z[n - M - 1], np.log(np.finfo(np.float64).tiny))
    assert np.array_equal(res["tail_len"], (z > c).sum(axis=0)), (tag, "tail_len")


# ---- ESS and band ESS: the passes and the checks of the lag products and the finish ----

def run_ess(acc, pushes, max_lag=0, block=0, ess_pushes=None, acov=True):
    """Fold pass over `pushes`, ESS pass over `ess_pushes` (default: the same pushes).  Returns the dict of ess_result()
    with acov_M, acov_l, the fold result under "fold" and the logL / status of both passes."""
    with capi.Summary(acc, block) as s:
        out0 = [s.push(P) for P in pushes]
        fold = s.result()
        lag = s.ess_begin(max_lag)
        out1 = [s.push(P) for P in (pushes if ess_pushes is None else ess_pushes)]
        r = s.ess_result()
        assert r["lag"] == lag
        if acov:
            r["acov_M"], r["acov_l"] = s.ess_acov(0), s.ess_acov(1)
        assert same(s.result(), fold), "the fold results changed in ESS mode"
        s.ess_end()
    r["fold"] = fold
    for k, o in (("fold_out", out0), ("ess_out", out1)):
        r[k] = (np.concatenate([a[0] for a in o]), np.concatenate([a[1] for a in o]))
    return r


def ulps(a, b):
    """max |a - b| in ulps of b; NaN must meet NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    if not ok.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        d = np.where(a[ok] == b[ok], 0.0, np.abs(a[ok] - b[ok]) / np.spacing(np.abs(b[ok])))
    return float(np.max(d))


ESS_WORST = {}


def check_acov(tag, res, rows, y, like=0, p=1.0, sigma=None, sel=None):
    """Case 1: ess_acov against the long-double lag products of the GPU's own rows (on the bins `sel`)."""
    sel = np.arange(rows.shape[1]) if sel is None else np.asarray(sel)
    fold, L = res["fold"], res["lag"]
    sg = None if sigma is None else sigma[sel]
    a, u, e_a, e_u = R.series(rows[:, sel], y[sel], fold["mean_M"][sel], fold["lppd"][sel], like, p, sg)
    ratios = {}
    for name, d, e in (("acov_M", a, e_a), ("acov_l", u, e_u)):
        A, bound = R.lag_products(d, e, L)
        got = res[name][:, sel]
        assert got.shape == A.shape and np.all(np.isfinite(got)), (tag, name)
        err = np.abs(got.astype(LD) - A).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(bound > 0, err / (10.0 * bound), np.where(err == 0, 0.0, np.inf))
        ratios[name] = float(ratio.max())
    print(f"RATIO ess {tag} L={L}: " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
    for k, v in ratios.items():
        ESS_WORST[k] = max(ESS_WORST.get(k, 0.0), v)
        assert v <= 1.0, (tag, k, v)


def check_finish(tag, res, rows=None):
    """Case 2: the finish in numpy float64 on the library's own lag products, and the totals."""
    fold, n, L = res["fold"], res["n_used"], res["lag"]
    assert n == fold["n_used"] and res["n_rejected"] == fold["n_rejected"] and L == res["acov_M"].shape[0] - 1
    tau_M, ess_M, cut_M = R.finish(res["acov_M"], n)
    _, ess_l, cut_l = R.finish(res["acov_l"], n)
    assert np.array_equal(res["cut_M"], cut_M) and np.array_equal(res["cut_l"], cut_l), tag
    with np.errstate(invalid="ignore"):
        want = dict(tau_M=tau_M, ess_M=ess_M, ess_l=ess_l, mcse_M=np.sqrt(fold["var_M"] / ess_M), r_eff=ess_l / np.float64(n))
    worst = {k: ulps(res[k], v) for k, v in want.items()}
    print(f"ULPS ess {tag} L={L}: " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 4.0, (tag, k, v)
    if rows is not None:
        ref = R.rhat(rows)
        got = np.asarray(res["rhat_M"]).astype(LD)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), tag
        ok = ~np.isnan(ref)
        rel = float(np.max(np.abs(got[ok] - ref[ok]) / ref[ok])) if ok.any() else 0.0
        print(f"RHAT ess {tag}: max relative difference {rel:.3g}")
        assert rel <= 1e-12, (tag, rel)
    # totals: the first bin wins a tie, a NaN is skipped

    def first(v, fn):
        v = np.asarray(v, dtype=np.float64)
        if np.all(np.isnan(v)):
            return np.nan, -1
        k = int(fn(np.where(np.isnan(v), -np.inf if fn is np.argmax else np.inf, v)))
        return v[k], k
    for key, arr, fn in (("min_ess_M", res["ess_M"], np.argmin), ("min_ess_l", res["ess_l"], np.argmin), ("max_rhat", res["rhat_M"], np.argmax)):
        v, k = first(arr, fn)
        assert bits(res[key]) == bits(v) and res["bin_" + key] == k, (tag, key)
    assert res["n_truncated_M"] == int((res["cut_M"] == L + 1).sum()) and res["n_truncated_l"] == int((res["cut_l"] == L + 1).sum()), tag
    with np.errstate(invalid="ignore"):
        assert res["n_rhat_high"] == int((res["rhat_M"] > 1.01).sum()), tag


def band_pass(s, pushes, thr, max_lag=0, counts=True):
    """One pass inside an open summary: begin, the pushes, result (and counts), end."""
    lag = s.bandess_begin(thr, max_lag)
    out = [s.push(P) for P in pushes]
    r = s.bandess_result()
    assert r["lag"] == lag
    if counts:
        ce = [s.bandess_counts(j) for j in range(r["n_thresholds"])]
        r["C"], r["E"] = [a for a, _ in ce], [b for _, b in ce]
    s.bandess_end()
    r["band_out"] = (np.concatenate([a[0] for a in out]), np.concatenate([a[1] for a in out]))
    return r


def order_stats(rows, levels):
    return np.sort(rows, axis=0)[ranks_of(levels, len(rows))]


# ---- the command-line tool ----

def stored_chain(tmp_path):
    """A 50-sample chain of slice 1 of the reference's real spectrum (the golden local-model inputs), written into tmp_path
    by the phase driver with the oracle as evaluator (as tests/test_outputs.py), and what chainsummary_hip is asked to read
    of it: samples 4, 6, ..., 48.  Returns the setup, the chain's root name, the 50 x Nvars stored variables, the 23
    parameter rows of the selection, the tool's leading arguments `common` (the output file comes next) and the selection's
    arguments `sel`."""
    from tamcmc_amd import outputs as O
    from tamcmc_amd import sampler as S
    from tamcmc_amd.setup_io import Setup
    model, data, out = MODEL, DATA, str(tmp_path) + "/"
    s = Setup(CFG).load(model, data, 0)
    s.set("MALA", "Nchains", 2)
    for k, v in (("output_dir", out), ("restore_dir", out), ("output_root_name", "TF_A_"), ("Nbuffer", 50), ("file_format", "binary")):
        s.set("Outputs", k, v)
    s.set("MALA", "Nt_learn", "10, 30, 100000")
    s.apply_phase("Burn-in", 50, 1.8)
    orc = pyorc()

    def ev(P, T):
        return orc.generate_batch(s.model_case, s.plength, s.x, s.y, P, T, likelihood_p=s.likelihood_p)[:2]
    smp = S.Sampler(s.sampler_cfg(seed=5), ev, s.plength, s.inputs, s.relax, s.err, s.priors_names_switch, s.priors, s.extra_priors)
    O.run_phase(s, smp)
    root = out + "TF_A_params"
    v, _ = O.read_params_bin(root, 0)
    rows = np.tile(s.inputs, (23, 1))
    rows[:, s.index_to_relax] = v[4::2]                       # update_params_with_vars, model_def.cpp:370-378
    return s, root, v, rows, [tool(), CFG, model, data, root], ["--thin", "2", "--first", "4", "--block", "7"]


def header_values(lines):
    """name -> text of every `name= value` pair of the given `#` lines."""
    val = {}
    for line in lines:
        tok = line[1:].split()
        val.update({a[:-1]: b for a, b in zip(tok, tok[1:]) if a.endswith("=")})
    return val


def f12(a):
    """The values as the tool prints them: 12 significant digits."""
    return np.array([float("%.12g" % t) for t in np.atleast_1d(a)])


# ---- the header's prototypes (host suites) ----

def prototypes():
    """name -> list of parameter types as the header spells them (comments and names stripped)."""
    txt = open(os.path.join(ROOT, "include", "tamcmc_accel.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(tamcmc_summary_[a-z_]+)\s*\(([^)]*)\)\s*;", txt):
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            a = re.sub(r"\s*\b[A-Za-z_]\w*$", "", a) if not a.endswith("*") else a      # drop the parameter's name
            types.append(a.replace(" *", "*"))
        out[name] = types
    return out, txt
