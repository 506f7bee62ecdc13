"""LOO-PIT of a stored chain on the GPU (tamcmc_summary_loo_pit_*, include/tamcmc_accel.h; tamcmc_loopit.hip): per bin the
predictive tail probabilities averaged with the Pareto-smoothed importance weights of PSIS-LOO, and Kish's effective sample
size of those weights, from a third pass over the samples of the fold pass.

Reference: loopit_reference() of tests/loopit_reference.py, an independent numpy transcription of the definition in the
header, run in long double.

Exact checks (no tolerance): every result is bitwise independent of block_chains (1, 7, 64, the default) and of the split of
the third pass into pushes, pushes of one sample included; host and device pointers give the same bits; a chain with
rejected rows gives the bits of the chain without them; loo_result returns the same bits before loo_pit_begin, after it and
after the pass; the fold, predictive, window and scan results keep their bytes; the totals are their stated expressions on
the returned arrays.

Against the reference on the GPU's own model rows the bound is, per case and per quantity (the maximum over the bins;
relative to max(1, |value|), absolute for loo_pit), 10 x the larger of
    (a) the reference's own change when the rows AND x = -l are each perturbed by 2^-50 relative, one sign per distinct row
        and bin (duplicated rows stay exact ties), the maximum over three seeds -- x is perturbed apart from the rows because
        near y = M it is insensitive to the row while its rounding is not -- and
    (b) the difference between the reference run in float64 and in long double.
Both must agree with the GPU on where a value is finite.  On the oracle's rows the perturbation is 1e-12 relative, the
project's per-bin model bar.  The identities are checked with the same bounds: |exp(loo_log_cdf) + exp(loo_log_sf) - 1|
within the slack of summary_support.check_tails_reference; the GPU's log_wsum against the reference's log(sum_body exp z +
sum_T exp zt); the reference's lse(lw - x) - lW against the GPU's elpd_loo; 1 <= is_ess <= n up to rounding.
Every worst ratio is printed before it is asserted (pytest -s).

Worst ratios observed on an MI355X over all cases below: on the GPU's own rows loo_log_cdf 0.10 (2 bins, 37 samples),
loo_log_sf 0.088, loo_pit 0.13, is_ess 0.082, log_wsum 0.034, elpd_loo against the reference's weights 0.094; at 70 001
samples 0.011, 0.016, 0.017, 0.017, 0.0038 and 1.3e-4; on the oracle's rows 1.0e-3, 5.0e-4, 8.2e-4, 3.5e-5, 9.1e-6 and
4.8e-4.  The planted bin: loo_log_sf = -5.99658 against the posterior check's -5.99393, and the lowest is_ess (399.1 of 400).
"""
import numpy as np
import pytest

import workloads as W
from loopit_support import PIT_ARRAYS, PIT_TOTALS, check_reference, check_totals, run_pit, same_loo, same_pit
from summary_support import (ULP, c2_case, c2_chain, gpu_rows, other_cases, row_groups, same, same_pred, same_scans, same_win, spectrum_for,
                             tail_M, true_model)
from support import bits, in_torch_process, pyorc
from tamcmc_amd import capi, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("Nx", [2, 63, 64, 65, 257, 700])
def test_grid_ends(accel_mod, Nx):
    """One bin per thread in waves of 64 (PIT kernel), one wave per bin (prepare): a partial wave, exactly one, one and a
    bin, several.  37 samples: M = 8, a search of 4 steps."""
    w, y, P, _, _ = c2_case(Nx)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        res, loo, _ = run_pit(acc, [P])
        one, _, _ = run_pit(acc, [P], 1, [P[k:k + 1] for k in range(len(P))])
    assert same_pit(res, one), "block of 1, pushes of 1"
    assert res["n_used"] == 37 and res["n_rejected"] == 0 and np.all(loo["tail_len"] == 8)
    check_totals(f"grid-ends Nx={Nx}", res)
    check_reference(f"grid-ends Nx={Nx}", res, loo, rows, y, np.arange(len(P)), 2.0 ** -50)


@pytest.mark.parametrize("S", [1, 4, 20, 21, 26, 100, 400, 441, 455, 456])
def test_sample_counts_exact_and_reference(accel_mod, S):
    """n = 1 has no tail rule; up to n = 20 the tail holds at most 4 values and the weights are raw; n = 21 is the first
    chain with a Pareto fit.  441, 455 and 456 samples give M = 63, 64 and 65: 64, 65 and 66 slots, either side of a step of
    the search's trip count (6, 7, 7)."""
    w, y, P = c2_chain(65, S)
    if S >= 441:
        assert tail_M(S) == {441: 63, 455: 64, 456: 65}[S]
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        first, loo, _ = run_pit(acc, [P], 1)
        for B in (7, 64, 0):
            res, loo_b, _ = run_pit(acc, [P], B)
            assert same_pit(res, first) and same_loo(loo_b, loo), ("block_chains", B)
        a, b = S // 3, S // 3 + 1
        split = [P[:a], P[a:b], P[b:]] if S >= 3 else [P[k:k + 1] for k in range(S)]
        if 3 <= S <= 26:
            split = [P[k:k + 1] for k in range(S)]
        res, _, _ = run_pit(acc, [P], 7, [q for q in split if len(q)])
        assert same_pit(res, first), "the third pass split into pushes"
    check_totals(f"S={S}", first)
    check_reference(f"S={S}", first, loo, rows, y, np.arange(S), 2.0 ** -50)
    if S <= 20:
        assert np.all(np.isposinf(loo["pareto_k"]))
    if S == 1:                                                  # one sample: weight 1, the tails are that sample's
        assert np.all(first["is_ess"] == 1.0) and np.all(first["log_wsum"] == 0.0)


@pytest.mark.parametrize("name", ["c1-id11-fused", "p=2", "p=3", "chi-square-id2"])
def test_other_paths(accel_mod, name):
    """A local model on the fused one-tile launch (id 11), likelihood_p = 2 and 3 (the looped tails), and chi_square."""
    if name == "p=3":
        w, P, kw = W.make(2, Nx=3000), None, dict(p=3.0)
    else:
        w, P, kw = other_cases()[name]
    mid = w["model_case"]
    if P is None:
        P = synth.chain_params(w, 37) if "err" in w else W.perturbed(w, 37, scale=0.003)
    y = spectrum_for(w)
    like, p, sigma = kw.get("like", 0), kw.get("p", 1.0), kw.get("sigma")
    with accel_mod.Accel(mid, w["plength"], w["x"], y, sigma_y=sigma, likelihood_case=like, likelihood_p=p) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0), name
        res, loo, _ = run_pit(acc, [P], 8)
        other, _, _ = run_pit(acc, [P], 0, [P[:5], P[5:6], P[6:]])
        with capi.Summary(acc, 8, predictive=True) as s:
            s.push(P)
            post = s.predictive_result()
    assert same_pit(res, other), name
    check_totals(name, res)
    sel = np.arange(0, acc.Nx, max(acc.Nx // 65, 1))            # the reference on about 65 bins: the exact checks cover every bin
    check_reference(name, res, loo, rows, y, np.arange(len(P)), 2.0 ** -50, like, int(p), sigma, sel=sel)
    # LOO moves each tail by less than the posterior check's tail is from certainty, in nearly every bin: a smoke test of scale
    assert np.median(np.abs(np.asarray(res["loo_pit"]) - np.asarray(post["pit"]))) < 0.1, name


def test_ties(accel_mod):
    """Every row twice in a row (every rejected Metropolis proposal does that), one row 50 times, and all rows equal.  Every
    tail sample is found -- loo_pit_result would refuse otherwise -- equal rows may come in any order, and with all rows
    equal there is no tail (L = 0): the weights are equal and the result is the posterior check's."""
    w, y, P = c2_chain(65, 60)
    P2 = np.repeat(P, 2, axis=0)
    P50 = np.concatenate([P[:30], np.tile(P[7], (50, 1)), P[30:]])
    Pe = np.tile(P[5], (50, 1))
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        for tag, Q in (("twice", P2), ("fifty", P50)):
            _, st, rows = gpu_rows(acc, Q)
            assert np.all(st == 0)
            res, loo, _ = run_pit(acc, [Q], 16)
            other, _, _ = run_pit(acc, [Q], 1, [Q[:1], Q[1:3], Q[3:]])
            assert same_pit(res, other), tag
            check_totals(tag, res)
            check_reference(f"ties-{tag}", res, loo, rows, y, row_groups(Q), 2.0 ** -50)
        # the fifty equal rows first or last: the result does not depend on which of two equal samples came first -- the
        # sums run in push order, so this is within the bound, not bit for bit
        Q = np.concatenate([np.tile(P[7], (50, 1)), P])
        _, st, rows = gpu_rows(acc, Q)
        res, loo, _ = run_pit(acc, [Q], 16)
        check_reference("ties-fifty-first", res, loo, rows, y, row_groups(Q), 2.0 ** -50)
        eq, loo_eq, _ = run_pit(acc, [Pe], 7)
        with capi.Summary(acc, 7, predictive=True) as s:
            s.push(Pe)
            post = s.predictive_result()
    assert np.all(loo_eq["tail_len"] == 0)
    n = 50
    for a, b in (("loo_log_cdf", "log_cdf"), ("loo_log_sf", "log_sf")):
        assert np.all(np.abs(eq[a] - post[b]) <= (n + 2) * ULP), (a, float(np.max(np.abs(eq[a] - post[b]))))
    assert np.all(np.abs(eq["is_ess"] - n) <= n * (n + 2) * ULP) and np.all(np.abs(eq["log_wsum"] - np.log(50.0)) <= 2.0 * np.spacing(np.log(50.0)))


def test_rejected_samples(accel_mod):
    """A NaN parameter and an empty truncation window among 30 healthy samples, first and last in the chain, at block edges
    and alone in a block of one: left out of every bin, counted, and the bits are those of the chain without them."""
    w = W.make(2, Nx=3000)
    b = W.split(w)
    y = spectrum_for(w)
    good = W.perturbed(w, 30, scale=0.002)
    empty = W.perturbed(w, 1, scale=0.002, seed=8)[0]
    empty[b["q"] + 1] = -1.0
    nan = W.perturbed(w, 1, scale=0.002, seed=9)[0]
    nan[b["z"] + 9] = np.nan
    P = np.array([empty] + list(good[:3]) + [nan, nan] + list(good[3:25]) + [empty] + list(good[25:]) + [nan])
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, stg, rows = gpu_rows(acc, good)
        assert np.all(stg == 0)
        clean, loo, _ = run_pit(acc, [good], 3)
        for B in (4, 1, 0):                                     # B = 4: rejected rows at 0, 4 and 5 -- a block's first and second
            res, _, _ = run_pit(acc, [P], B)
            assert res["n_used"] == 30 and res["n_rejected"] == 5
            for k in PIT_ARRAYS + PIT_TOTALS[2:]:
                assert np.array_equal(bits(np.asarray(res[k], dtype=np.float64)), bits(np.asarray(clean[k], dtype=np.float64))), (B, k)
            assert np.array_equal(res["loo_pit_hist"], clean["loo_pit_hist"])
    sel = np.arange(0, 3000, 46)
    check_reference("rejected", clean, loo, rows, y, np.arange(30), 2.0 ** -50, sel=sel)


@pytest.mark.parametrize("name", ["c2-65-S400-scale3", "c2-700-S200-scale3", "c2-700-S37", "triples"])
def test_against_the_oracle(accel_mod, name):
    """The LOO suite's four cases on the oracle's rows: the perturbation is the project's per-bin model bar."""
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
        res, loo, _ = run_pit(acc, [P])
    check_totals(name, res)
    check_reference(f"oracle {name}", res, loo, M, y, row_groups(P), 1e-12)


def test_planted_outlier(accel_mod):
    """One bin's datum at 6 x the model: the posterior check averages over a chain that has seen it, LOO-PIT does not, so its
    survival probability is lower there; and the weights are least even near it.  The spectrum is the model times
    exponential draws capped at 3 (the usual synthetic spectrum has draws of 20 of its own), and the bin is chosen, from the
    oracle's rows, where the model varies most over the chain: to first order the log weight x = y / M + log M varies by
    (y / M - 1) d log M, so with y / M = 6 there and (y / M - 1)^2 var(log M) smaller by a factor of 3 everywhere else --
    asserted -- that bin's weights are the least even."""
    w, y0, P = c2_chain(257, 400)
    _, rst, M = pyorc().generate_batch(2, w["plength"], w["x"], y0, P, np.ones(len(P)), want_models=True)
    assert np.all(rst == 0)
    Mt = true_model(w)
    v = np.var(np.log(M), axis=0)
    k = 2 + int(np.argmax(v[2:-2]))
    y = Mt * np.minimum(np.random.default_rng(5).exponential(size=Mt.size), 3.0)
    y[k] = 6.0 * Mt[k]
    score = (y / M.mean(axis=0) - 1.0) ** 2 * v
    far = np.abs(np.arange(Mt.size) - k) > 2
    assert np.all(3.0 * score[far] < score[k]), (k, float(score[k]), float(score[far].max()))
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        res, _, _ = run_pit(acc, [P], 64, predictive=True)
        with capi.Summary(acc, 64, predictive=True) as s:
            s.push(P)
            post = s.predictive_result()
    print(f"PLANTED bin {k}: loo_log_sf = {res['loo_log_sf'][k]:.6g}, posterior log_sf = {post['log_sf'][k]:.6g}, is_ess = {res['is_ess'][k]:.6g}, "
          f"min_is_ess = {res['min_is_ess']:.6g} at bin {res['bin_min_is_ess']}")
    assert res["loo_log_sf"][k] < post["log_sf"][k]
    assert abs(res["bin_min_is_ess"] - k) <= 2


def test_other_results_keep_their_bytes(accel_mod):
    """The fold, predictive, window and scan results of an object are the same bytes before LOO mode, inside the LOO-PIT
    sub-mode after a pass, and after loo_end."""
    w, y, P, _, _ = c2_case(257)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        with capi.Summary(acc, 16, predictive=True, window=(16, 5), scan=(4, 16)) as s:
            s.push(P)
            before = (s.result(), s.predictive_result(), s.window_result(), [s.scan_result(k) for k in range(2)])

            def unchanged(where):
                now = (s.result(), s.predictive_result(), s.window_result(), [s.scan_result(k) for k in range(2)])
                assert same(now[0], before[0]) and same_pred(now[1], before[1]) and same_win(now[2], before[2]) and \
                    same_scans(now[3], before[3]), where
            s.loo_begin()
            s.push(P)
            s.loo_pit_begin()
            unchanged("after loo_pit_begin")
            s.push(P)
            s.loo_pit_result()
            unchanged("after the PIT pass")
            s.loo_end()
            unchanged("after loo_end")


def test_refusals_and_state(accel_mod):
    w, y, P, _, _ = c2_case(257)
    T = np.ones(len(P))
    E = capi.E_INVALID
    extra = synth.chain_params(w, 5, seed=4242)
    others = synth.chain_params(w, len(P), seed=977)            # as many rows, other rows

    def refused(fn, *a):
        with pytest.raises(accel_mod.AccelError) as e:
            fn(*a)
        assert e.value.code == E

    acc = accel_mod.Accel(2, w["plength"], w["x"], y)
    clean, clean_loo, _ = run_pit(acc, [P])
    s = capi.Summary(acc, 8)
    refused(s.loo_pit_begin)                                                 # outside LOO mode: empty, and after a fold pass
    refused(s.loo_pit_result)
    s.push(P)
    full = s.result()
    refused(s.loo_pit_begin)
    s.loo_begin()
    refused(s.loo_pit_begin)                                                 # nothing pushed in LOO mode
    s.push(P[:20])
    refused(s.loo_pit_begin)                                                 # the pass is incomplete -- and survives:
    s.push(P[20:])                                                           # pushing the rest completes it
    assert same_loo(s.loo_result(), clean_loo), "the LOO pass did not survive a refused loo_pit_begin"
    acc.begin(P, T)                                                          # a batch in flight
    refused(s.loo_pit_begin)
    acc.end()
    acc.arm(len(P))                                                          # a batch armed
    refused(s.loo_pit_begin)
    acc.disarm()
    refused(s.loo_pit_result)                                                # not begun
    s.loo_pit_begin()
    refused(s.loo_pit_begin)                                                 # twice
    refused(s.loo_pit_result)                                                # nothing pushed
    s.push(P[:-1])                                                           # a pass of S - 1 samples
    refused(s.loo_pit_result)
    s.push(P)
    s.push(P[3:4])                                                           # one sample too many
    refused(s.loo_pit_result)
    s.push(others)                                                           # S other rows: the counts are right, the tail samples are not found
    refused(s.loo_pit_result)
    s.push(P[:20])                                                           # the right pass, in two pushes
    s.push(P[20:])
    assert same_pit(s.loo_pit_result(), clean), "after discarded passes"
    assert same_loo(s.loo_result(), clean_loo)
    assert same(s.result(), full)
    s.loo_end()
    refused(s.loo_pit_result)
    refused(s.loo_pit_begin)
    s.push(extra)                                                            # folds on as if nothing had happened
    after = s.result()
    with capi.Summary(acc, 8) as s2:
        s2.push(P)
        s2.push(extra)
        assert same(s2.result(), after), "a summary that never entered the sub-mode differs"
    allP = np.concatenate([P, extra])
    d = s.loo(allP, pit=True)                                                # the convenience call leaves the mode
    assert d["n_used"] == len(P) + 5 and all(k in d for k in PIT_ARRAYS + ("elpd_loo", "pareto_k"))
    assert set(s.loo(allP)) == set(capi.Summary.LOO_ARRAYS + ("tail_len",) + capi.Summary.LOO_TOTALS)      # the default keeps its dict
    refused(s.loo_end)
    s.loo_begin()
    s.push(allP)
    s.loo_pit_begin()
    s.push(P[:9])
    s.reset()                                                                # leaves the sub-mode and the mode, forgets every sample
    refused(s.loo_pit_result)
    refused(s.loo_result)
    assert s.result()["n_used"] == 0
    s.push(P)
    assert same(s.result(), full)
    s.loo_begin()
    s.push(P)
    s.loo_pit_begin()
    s.push(P[:9])
    refused(acc.close)                                                       # a live summary holds the context
    s.close()                                                                # inside the sub-mode, a pass half pushed
    acc.close()
    # chi(2,2p) with p outside 1 ... 64: LOO mode works, the sub-mode is refused
    with accel_mod.Accel(2, w["plength"], w["x"], y, likelihood_p=65.0) as acc65:
        with capi.Summary(acc65, 8) as s:
            s.push(P)
            s.loo_begin()
            s.push(P)
            s.loo_result()
            refused(s.loo_pit_begin)


def test_at_length(accel_mod):
    """70 001 samples of a 65-bin grid in blocks of 4096: M = 794, a search of 10 steps down a column of 795 slots, 17 pushes
    of blocks that straddle 65 535.  The reference runs on every eighth bin."""
    S = 70001
    w = synth.workload_c2(Nx=65)
    y = spectrum_for(w)
    P = synth.chain_params(w, S)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        with capi.Summary(acc, 4096) as s:
            s.push(P)
            res = s.loo(P, pit=True)
    assert tail_M(S) == 794 and res["n_used"] == S and np.all(res["tail_len"] == 794)
    check_totals("at-length", res)
    check_reference("at-length", res, res, rows, y, np.arange(S), 2.0 ** -50, sel=np.arange(0, 65, 8))


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
            host = s.loo(P, pit=True)
        acc.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        dP = torch.from_numpy(np.ascontiguousarray(P)).to(dev)
        dL = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
        dS = torch.full((n,), -9, dtype=torch.int32, device=dev)
        with capi.Summary(acc, 64) as s:
            s.push_device(n, dP.data_ptr())
            s.loo_begin()
            s.push_device(n, dP.data_ptr())
            s.loo_pit_begin()
            s.push_device(10, dP.data_ptr(), dL.data_ptr(), dS.data_ptr())   # enqueued, no sync; with and without outputs
            s.push_device(n - 10, dP[10:].data_ptr(), dL[10:].data_ptr(), dS[10:].data_ptr())
            r = s.loo_pit_result()
            assert same_pit(r, host)
            assert np.array_equal(bits(dL.cpu().numpy()), bits(L0)) and np.array_equal(dS.cpu().numpy(), st0)
            s.loo_end()
        acc.set_stream(0)
    print("loopit device path ok")


def test_device_pointers():
    in_torch_process("test_summary_loopit_gpu", "_device_check", "loopit device path ok")
