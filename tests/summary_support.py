"""What two or more of the posterior-summary suites use (tests/test_summary_*_gpu.py, tests/test_cli_*_gpu.py,
tests/test_scan_null_gpu.py, tests/test_summary_*_host.py): the cases and their references, the bit-for-bit comparisons, the
common body of the three tail checks, and the stored chain of the command-line tests.  Importing this module needs no GPU.

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
