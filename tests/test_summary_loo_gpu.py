"""PSIS-LOO of a stored chain on the GPU (tamcmc_summary_loo_*, include/tamcmc_accel.h; tamcmc_loo.hip): per bin the
leave-one-out log predictive density by Pareto-smoothed importance sampling and the Pareto shape k-hat, from one more pass
over the samples of the fold pass.

Reference: psis_reference() of tests/summary_support.py, an independent numpy transcription of the definition in the header, run in long double.

Exact checks (no tolerance): the library's own l_is, bit for bit, is mean_l of a summary that folded that sample alone; the
cutoff must be the (M+1)-th largest -l, bit for bit -- which also pins that the tail kernel's restated formulas for l agree
with the fold kernel's; tail_len must be the count of z strictly above the (floored) cutoff; everything must be bitwise
independent of block_chains and of the split into pushes.

Against the reference on the GPU's own model rows (eval_batch with every chain in model_rows) the bound is, per case and
per quantity (elpd_loo_i, k-hat_i; the maximum over the bins), 10 x the larger of
    (a) the reference's own change when every x is perturbed by 2^-50 relative (one random sign per value), and
    (b) the difference between the reference run in float64 and in long double.
The factor 10: one random perturbation samples the typical sensitivity, not the worst.
Against the reference on the oracle's rows (pyoracle.generate_batch(..., want_models=True)) the perturbation is 1e-12
relative -- the project's per-bin model bar -- one factor per distinct parameter row and bin (duplicated rows must stay
exact ties: independent factors on duplicates move k-hat by 2e-2), the maximum over bins and five seeds, and the bound is
10 x that change.  Every worst ratio is printed before it is asserted (pytest -s).

Worst ratios observed on an MI355X over all cases below: on the GPU's own rows elpd_loo 0.10 (several cases, the
70 001-sample one among them), k-hat 0.070 (likelihood_p = 2); on the oracle's rows elpd_loo 1.5e-4 (triples), k-hat
2.3e-5 (700 bins, 200 samples, scale 3).
"""
import subprocess

import numpy as np
import pytest

import workloads as W
from summary_support import (c2_case, c2_chain, exact_structure, f12, gpu_rows, header_values, library_l, other_cases, row_groups,
                             same, spectrum_for, stored_chain, tail_M, x_of)
from summary_support import check_loo_reference as check_reference
from support import LD, bits, in_torch_process, pyorc
from tamcmc_amd import capi, synth

pytestmark = pytest.mark.gpu

LOO_KEYS = ("elpd_loo", "pareto_k", "cutoff", "tail_len")
LOO_TOTALS = capi.Summary.LOO_TOTALS


def run_loo(acc, pushes, block=0):
    """Fold pass and LOO pass over the same pushes.  Returns (loo result, fold result, logL, status of the LOO pass)."""
    with capi.Summary(acc, block) as s:
        for P in pushes:
            s.push(P)
        fold = s.result()
        s.loo_begin()
        out = [s.push(P) for P in pushes]
        r = s.loo_result()
        assert same(s.result(), fold), "the fold results changed in LOO mode"
        s.loo_end()
    return r, fold, np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def same_loo(r1, r2):
    return all(np.array_equal(bits(r1[k]), bits(r2[k])) for k in LOO_KEYS[:3]) and np.array_equal(r1["tail_len"], r2["tail_len"]) and \
        all(np.array_equal(bits(float(r1[k])), bits(float(r2[k]))) for k in LOO_TOTALS)


@pytest.mark.parametrize("Nx", [2, 63, 64, 65, 257, 700])
def test_grid_ends(accel_mod, Nx):
    """One bin per thread in waves of 64 (tail kernel), one wave per bin (finalize): a partial wave, exactly one, one and a
    bin, several.  37 samples: M = 8, every k-hat finite."""
    w, y, P, _, _ = c2_case(Nx)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        res, fold, _, _ = run_loo(acc, [P])
    ref = check_reference(f"grid-ends Nx={Nx}", res, x_of(rows, y), np.arange(len(P)), 2.0 ** -50, (1,), x64=x_of(rows, y, dtype=np.float64))
    assert np.all(ref["tail_len"] == 8) and np.all(np.isfinite(ref["pareto_k"]))
    # p_loo is the difference of the two long-double sums, rounded once: within an ulp of each rounded total
    assert abs(res["p_loo"] - (fold["lppd_total"] - res["elpd_loo_total"])) <= 2.0 * np.spacing(abs(fold["lppd_total"]))
    assert res["n_used"] == 37 and res["n_rejected"] == 0


@pytest.mark.parametrize("S", [1, 4, 20, 21, 26, 100, 400])
def test_sample_counts_exact_and_reference(accel_mod, S):
    """n = 1 has no tail rule; up to n = 20 the tail holds at most 4 values and every k-hat is +inf; n = 21 is the first
    chain with a Pareto fit (M = 5)."""
    w, y, P = c2_chain(65, S)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        l = library_l(acc, P)
        first, fold, logL0, _ = run_loo(acc, [P], 1)
        for B in (7, 64):
            res, _, logL, _ = run_loo(acc, [P], B)
            assert same_loo(res, first), ("block_chains", B)
            assert np.array_equal(bits(logL), bits(logL0))
        if S >= 3:
            a, b = S // 3, S // 3 + 1
            res, _, _, _ = run_loo(acc, [P[:a], P[a:b], P[b:]], 7)
            assert same_loo(res, first), "three unequal pushes"
    exact_structure(f"S={S}", first, l)
    ref = check_reference(f"S={S}", first, x_of(rows, y), np.arange(S), 2.0 ** -50, (1,), x64=x_of(rows, y, dtype=np.float64))
    if S == 1:
        assert np.array_equal(first["elpd_loo"], fold["mean_l"]) and np.array_equal(first["elpd_loo"], l[0])
    if S <= 20:
        assert np.all(np.isposinf(first["pareto_k"])) and first["n_k_inf"] == 65 and first["k_max"] == np.inf
    if S == 21:
        assert tail_M(21) == 5 and np.all(ref["tail_len"] == 5) and np.all(np.isfinite(first["pareto_k"])) and first["n_k_inf"] == 0


@pytest.mark.parametrize("Nx,S,n_high", [(65, 400, 1), (700, 200, 6)])
def test_high_k(accel_mod, Nx, S, n_high):
    """A wide chain (scale = 3): bins on top of narrow modes whose importance ratios have a heavy tail.  The counts are asserted
    on the reference, so the cases cannot silently stop covering k-hat > 0.7."""
    w, y, P = c2_chain(Nx, S, 3.0)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        l = library_l(acc, P) if Nx == 65 else None
        res, _, _, _ = run_loo(acc, [P], 64)
    ref = check_reference(f"high-k Nx={Nx} S={S}", res, x_of(rows, y), np.arange(S), 2.0 ** -50, (1,), x64=x_of(rows, y, dtype=np.float64))
    assert int((ref["pareto_k"] > 0.7).sum()) == n_high, ref["pareto_k"][ref["pareto_k"] > 0.5]
    if Nx == 65:
        assert int((ref["pareto_k"] <= 0.5).sum()) == 64 and abs(float(ref["pareto_k"].max()) - 0.760) < 5e-4
        exact_structure("high-k", res, l)
    assert res["n_k_high"] == n_high and res["n_k_inf"] == 0


def test_ties_and_equal_samples(accel_mod):
    """Every row three times: exact ties at the cutoff are body, so L < M.  An all-equal chain: L = 0, k-hat = +inf."""
    w, y, P = c2_chain(65, 41)
    P3 = np.repeat(P, 3, axis=0)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P3)
        assert np.all(st == 0)
        l = library_l(acc, P3)
        res, _, _, _ = run_loo(acc, [P3], 16)
        Pe = np.tile(P[5], (50, 1))
        eq, fold, _, _ = run_loo(acc, [Pe], 7)
    assert tail_M(123) == 25
    exact_structure("triples", res, l)
    assert np.all(res["tail_len"] == 24)
    check_reference("triples", res, x_of(rows, y), row_groups(P3), 2.0 ** -50, (1,), x64=x_of(rows, y, dtype=np.float64))
    assert np.all(eq["tail_len"] == 0) and np.all(np.isposinf(eq["pareto_k"])) and eq["n_k_inf"] == 65
    assert np.array_equal(eq["cutoff"], -fold["mean_l"])
    # elpd = (log 50 - x) - log 50: two roundings of values no larger than log 50 + |l|
    assert np.all(np.abs(eq["elpd_loo"] - fold["mean_l"]) <= np.spacing(np.log(50.0) + np.abs(fold["mean_l"])))


def test_rejected_samples(accel_mod):
    """A NaN parameter and an empty truncation window among 30 healthy samples, first and last in a block and alone in a block
    of one: left out of every bin, counted, and the logL / status bits of the LOO pass are the fold pass's."""
    w = W.make(2, Nx=3000)
    b = W.split(w)
    y = spectrum_for(w)
    good = W.perturbed(w, 30, scale=0.002)
    empty = W.perturbed(w, 1, scale=0.002, seed=8)[0]
    empty[b["q"] + 1] = -1.0
    nan = W.perturbed(w, 1, scale=0.002, seed=9)[0]
    nan[b["z"] + 9] = np.nan
    P = np.array([empty] + list(good[:2]) + [nan, nan] + list(good[2:25]) + [empty] + list(good[25:]))
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, stg, rows = gpu_rows(acc, good)
        assert np.all(stg == 0)
        clean, _, _, _ = run_loo(acc, [good], 3)
        for B in (4, 1):
            with capi.Summary(acc, B) as s:
                L0, st0 = s.push(P)
                s.loo_begin()
                L1, st1 = s.push(P)
                res = s.loo_result()
            assert np.array_equal(bits(L1), bits(L0)) and np.array_equal(st1, st0) and sorted(st0[st0 != 0]) == [1, 1, 2, 2]
            assert res["n_used"] == 30 and res["n_rejected"] == 4
            for k in LOO_KEYS + LOO_TOTALS[2:]:
                assert np.array_equal(bits(np.asarray(res[k], dtype=np.float64)), bits(np.asarray(clean[k], dtype=np.float64))), (B, k)
    ref = check_reference("rejected", res, x_of(rows, y), np.arange(30), 2.0 ** -50, (1,), x64=x_of(rows, y, dtype=np.float64))
    assert np.all(np.isfinite(ref["pareto_k"]))


@pytest.mark.parametrize("name", ["c1-id11-fused", "p=2", "chi-square-id2"])
def test_other_paths(accel_mod, name):
    """One local model on the fused one-tile launch (id 11), likelihood_p = 2, and chi_square (l without the factor 1/2)."""
    w, P, kw = other_cases()[name]
    mid = w["model_case"]
    if P is None:
        P = synth.chain_params(w, 37) if "err" in w else W.perturbed(w, 37, scale=0.003)
    y = spectrum_for(w)
    like, p, sigma = kw.get("like", 0), kw.get("p", 1.0), kw.get("sigma")
    with accel_mod.Accel(mid, w["plength"], w["x"], y, sigma_y=sigma, likelihood_case=like, likelihood_p=p) as acc:
        if name == "c1-id11-fused":
            assert acc.geometry()["tiles"] == 1
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0), name
        sel = np.arange(0, acc.Nx, max(acc.Nx // 65, 1))
        l = library_l(acc, P)
        res, _, _, _ = run_loo(acc, [P], 8)
    exact_structure(name, res, l)
    assert np.all(res["tail_len"] <= 8) and np.any(res["tail_len"] == 8)      # (chi_square: x spreads over thousands, and where the cutoff's z is under log(DBL_MIN) the floor shortens the tail)
    # the reference on every 15th to 46th bin (about 65 of them): the exact checks above cover every bin
    sub = {k: np.asarray(res[k])[sel] for k in LOO_KEYS}
    sg = None if sigma is None else sigma[sel]
    check_reference(name, sub, x_of(rows[:, sel], y[sel], like, p, sg), np.arange(len(P)), 2.0 ** -50, (1,),
                    x64=x_of(rows[:, sel], y[sel], like, p, sg, dtype=np.float64), totals=False)
    assert res["elpd_loo_total"] == float(np.asarray(res["elpd_loo"]).astype(LD).sum())


@pytest.mark.parametrize("name", ["c2-65-S400-scale3", "c2-700-S200-scale3", "c2-700-S37", "triples"])
def test_against_the_oracle(accel_mod, name):
    if name == "triples":
        w, y, P = c2_chain(65, 41)
        P = np.repeat(P, 3, axis=0)
    elif name == "c2-700-S37":
        w, y, P, _, _ = c2_case(700)
    else:
        w, y, P = c2_chain(65, 400, 3.0) if name.startswith("c2-65") else c2_chain(700, 200, 3.0)
    _, rst, M = pyorc().generate_batch(2, w["plength"], w["x"], y, P, np.ones(len(P)), want_models=True)
    assert np.all(rst == 0)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        res, _, _, _ = run_loo(acc, [P])
    check_reference(f"oracle {name}", res, x_of(M, y), row_groups(P), 1e-12, (1, 2, 3, 4, 5))


def test_refusals_and_state(accel_mod):
    w, y, P, _, _ = c2_case(257)
    T = np.ones(len(P))
    E = capi.E_INVALID
    extra = synth.chain_params(w, 5, seed=4242)

    def refused(fn, *a):
        with pytest.raises(accel_mod.AccelError) as e:
            fn(*a)
        assert e.value.code == E

    acc = accel_mod.Accel(2, w["plength"], w["x"], y)
    clean, _, _, _ = run_loo(acc, [P])
    s = capi.Summary(acc, 8)
    refused(s.loo_begin)                                                     # before any push: n_used < 1
    refused(s.loo_result)
    refused(s.loo_end)
    s.push(P)
    full = s.result()
    s.quantiles_begin((0.16, 0.5, 0.84))
    refused(s.loo_begin)                                                     # in quantile mode
    s.quantiles_end()
    acc.begin(P, T)                                                          # a batch in flight
    refused(s.loo_begin)
    acc.end()
    acc.arm(len(P))                                                          # a batch armed
    refused(s.loo_begin)
    acc.disarm()
    s.loo_begin()
    refused(s.loo_begin)                                                     # twice in a row
    refused(s.quantiles_begin, (0.5,))                                       # quantile mode is refused in LOO mode
    refused(s.loo_result)                                                    # nothing pushed
    s.push(P[:-1])                                                           # a pass of S - 1 samples
    refused(s.loo_result)
    s.push(P)
    s.push(P[3:4])                                                           # one sample too many
    refused(s.loo_result)
    s.push(P[:20])                                                           # the full pass, in two pushes
    s.push(P[20:])
    r = s.loo_result()
    assert same_loo(r, clean), "after discarded passes"
    assert same_loo(s.loo_result(), clean), "a second result without another pass"
    assert same(s.result(), full)
    s.loo_end()
    refused(s.loo_result)
    refused(s.loo_end)
    s.push(extra)                                                            # folds on as if nothing had happened
    after = s.result()
    with capi.Summary(acc, 8) as s2:
        s2.push(P)
        s2.push(extra)
        assert same(s2.result(), after), "a summary that never entered the mode differs"
    d = s.loo(np.concatenate([P, extra]))                                    # the convenience call leaves the mode
    assert d["n_used"] == len(P) + 5
    refused(s.loo_end)
    s.loo_begin()
    s.push(P[:9])
    s.reset()                                                                # leaves the mode, forgets every sample
    refused(s.loo_result)
    assert s.result()["n_used"] == 0
    s.push(P)
    assert same(s.result(), full)
    s.loo_begin()
    s.push(P[:9])
    refused(acc.close)                                                       # a live summary holds the context
    s.close()                                                                # inside the mode, a pass half pushed
    acc.close()


def test_at_length(accel_mod):
    """70 001 samples of a 65-bin grid in blocks of 4096: M = 794, the heap's fill phase, tens of thousands of replacements
    and 17 pushes of blocks that straddle 65 535.  Folding every sample alone would take 70 001 pushes, so for this one case
    l comes from the GPU's rows in float64 with numpy's log -- which may differ from the device's log in the last bit, hence
    a cutoff within 4 ulp instead of bit for bit; tail_len stays exact (the values are distinct, so it is M)."""
    S = 70001
    w = synth.workload_c2(Nx=65)
    y = spectrum_for(w)
    P = synth.chain_params(w, S)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        with capi.Summary(acc, 4096) as s:
            s.push(P)
            res = s.loo(P)
    M = tail_M(S)
    assert M == 794 and res["n_used"] == S
    xs = np.sort(x_of(rows, y, dtype=np.float64), axis=0)
    cut = xs[S - M - 1]
    assert np.all(np.abs(res["cutoff"] - cut) <= 4 * np.spacing(np.abs(cut))), float(np.max(np.abs(res["cutoff"] - cut) / np.spacing(np.abs(cut))))
    z = xs - xs[-1]
    assert np.array_equal(res["tail_len"], (z > z[S - M - 1]).sum(axis=0)) and np.all(res["tail_len"] == M)
    check_reference("at-length", res, x_of(rows, y), np.arange(S), 2.0 ** -50, (1,), x64=xs)


def _device_check():
    """Body of test_device_pointers, in a process where torch owns the device first (as bench.py)."""
    import torch
    import tamcmc_amd as accel_mod
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    w, y, P = c2_chain(700, 200, 3.0)
    n = len(P)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        with capi.Summary(acc, 7) as s:
            L0, st0 = s.push(P)
            host = s.loo(P)
        acc.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        dP = torch.from_numpy(np.ascontiguousarray(P)).to(dev)
        dL = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
        dS = torch.full((n,), -9, dtype=torch.int32, device=dev)
        with capi.Summary(acc, 64) as s:
            s.push_device(n, dP.data_ptr())
            s.loo_begin()
            s.push_device(10, dP.data_ptr(), dL.data_ptr(), dS.data_ptr())   # enqueued, no sync; with and without outputs
            s.push_device(n - 10, dP[10:].data_ptr(), dL[10:].data_ptr(), dS[10:].data_ptr())
            r = s.loo_result()
            assert same_loo(r, host)
            assert np.array_equal(bits(dL.cpu().numpy()), bits(L0)) and np.array_equal(dS.cpu().numpy(), st0)
            s.loo_end()
        acc.set_stream(0)
    print("loo device path ok")


def test_device_pointers():
    in_torch_process("test_summary_loo_gpu", "_device_check", "loo device path ok")


def test_command_line(accel_mod, tmp_path):
    """The 23-sample chain of summary_support.stored_chain on the golden local-model inputs with --loo: one more header line
    and two last columns, the numbers Summary.loo gives to the 12 printed digits; everything else is, byte for byte, what the
    same binary writes without the flag."""
    s, root, v, rows, common, sel = stored_chain(tmp_path)
    with accel_mod.Accel(s.model_case, s.plength, s.x, s.y, sigma_y=s.sigma_y, likelihood_case=s.likelihood_case,
                         likelihood_p=s.likelihood_p) as acc:
        with capi.Summary(acc) as sm:
            _, st = sm.push(rows)
            d = sm.loo(rows)
    assert np.all(st == 0) and d["n_used"] == 23
    for extra, ncol in (([], 8), (["--quantiles", "0.16,0.5,0.84"], 11)):
        plain, table = str(tmp_path / f"plain{ncol}.txt"), str(tmp_path / f"loo{ncol}.txt")
        for path, flag in ((plain, []), (table, ["--loo"])):
            r = subprocess.run(common + [path] + sel + extra + flag, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout + r.stderr
        t = np.loadtxt(table)
        assert t.shape == (s.Nx, ncol + 2)
        assert np.array_equal(t[:, ncol], f12(d["elpd_loo"])) and np.array_equal(t[:, ncol + 1], f12(d["pareto_k"]))
        lines0, lines = open(plain).read().split("\n"), open(table).read().split("\n")
        added = [k for k, line in enumerate(lines) if line.startswith("# elpd_loo=")]
        assert len(added) == 1 and lines[added[0] - 1].startswith("# quantiles=" if extra else "# lppd_total=")
        head = header_values([lines[added[0]]])
        for k, key in (("elpd_loo", "elpd_loo_total"), ("p_loo", "p_loo"), ("looic", "looic"), ("k_max", "k_max")):
            assert head[k] == "%.12g" % d[key], k
        assert int(head["n_k_high"]) == d["n_k_high"] and int(head["n_k_inf"]) == d["n_k_inf"]
        # minus the added line and the two columns: the bytes of the run without the flag
        stripped = []
        for k, line in enumerate(lines):
            if k == added[0]:
                continue
            if line.startswith("# x y "):
                assert line.endswith(" elpd_loo pareto_k")
                line = line[:-len(" elpd_loo pareto_k")]
            elif line and not line.startswith("#"):
                line = line.rsplit(" ", 2)[0]
            stripped.append(line)
        assert stripped == lines0, "the output without --loo changed"
