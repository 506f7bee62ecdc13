"""Effective sample size, MCSE and split R-hat of a stored chain on the GPU (tamcmc_summary_ess_*, include/tamcmc_accel.h;
tamcmc_ess.hip): per bin the lag products of the two centred series over the accepted samples in push order, Geyer's
initial monotone sequence on them, and the split R-hat of the model series, from one more pass over the samples of the
fold pass.

Reference: tests/ess_reference.py, an independent numpy statement of the definition.

1. Lag products: the GPU's own model rows (eval_batch with every chain in model_rows) give both series and every A_k in
   long double; ess_acov must agree within 10 x the sensitivity derived in ess_reference.py (the accumulation term, one ulp
   in each centred value, and for the likelihood series one ulp in l and in exp).  Every worst ratio is printed before it is
   asserted (pytest -s).
2. The finish, exactly: the rule in plain numpy float64 on the library's own ess_acov and frozen var_M: equal cuts, and tau,
   ess, mcse, r_eff within 4 ulp (the operations are fixed, so 0 is expected; the slack covers the host's log10); R-hat
   within 1e-12 relative of the formula on the GPU's rows.
3. Invariance, bit for bit: block_chains, the split into pushes (different in the two passes), rejected samples, host against
   device pointers.
4. Nothing else moves: the fold, predictive and window results keep their bytes before, during and after the mode.
5. Known answers: a chain that moves only the white-noise level N0 as an AR(1) sequence.
6. The protocol: every refusal, a short pass, mutual exclusion with the other modes, reset and destroy inside the mode.

Worst ratios to the bound observed on an MI355X over all cases below: see README.md ("Effective sample size").
"""
import numpy as np
import pytest

import ess_reference as R
from summary_support import c2_chain, check_acov, check_finish, gpu_rows, run_ess, same, spectrum_for
from support import bits, in_torch_process
from tamcmc_amd import capi, synth

pytestmark = pytest.mark.gpu

ESS_KEYS = capi.Summary.ESS_ARRAYS
ESS_TOTALS = capi.Summary.ESS_TOTALS
PRED_KEYS = capi.Summary.PREDICTIVE_ARRAYS + capi.Summary.PREDICTIVE_TOTALS + ("pit_hist",)
WIN_KEYS = capi.Summary.WINDOW_ARRAYS + capi.Summary.WINDOW_TOTALS + ("pit_hist",)


def same_ess(r1, r2, skip=()):
    keys = [k for k in ESS_KEYS + ESS_TOTALS + ("acov_M", "acov_l") if k not in skip and k in r1 and k in r2]
    return all(np.array_equal(bits(np.asarray(r1[k], dtype=np.float64)), bits(np.asarray(r2[k], dtype=np.float64))) for k in keys) and \
        all(np.asarray(r1[k]).shape == np.asarray(r2[k]).shape for k in keys)


@pytest.mark.parametrize("n", [4, 5, 64, 1000])
@pytest.mark.parametrize("Nx", [2, 65, 700])
def test_lag_products_and_finish(accel_mod, Nx, n):
    """Cases 1 and 2 on id 2, chi(2,2p) with p = 1: a partial wave of bins, one and a bin, several workgroups; chains of 4 and 5
    samples (L = 3 whatever is asked), 64 (one chunk exactly; L = 63 is the clipping case) and 1000; max_lag 1, 3, 63, 255 and
    1023, which n - 1 clips.  The largest shape, 700 bins and 1000 samples, runs L = 1 and 255 only: 3 and 63 are covered at
    700 bins by the shorter chains and at 1000 samples by the smaller grids, and so are the 999 lags that 1023 resolves to,
    whose long-double reference alone would take most of a minute there."""
    w, y, P = c2_chain(Nx, n)
    done = set()
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        for max_lag in (1, 3, 63, 255, 1023, 0):
            L = R.lag_limit(max_lag, n)
            if L in done or (Nx == 700 and n == 1000 and L not in (1, 255)):
                continue
            done.add(L)
            res = run_ess(acc, [P], max_lag)
            assert res["lag"] == L and res["n_used"] == n and res["n_rejected"] == 0
            tag = f"Nx={Nx} n={n}"
            check_acov(tag, res, rows, y)
            check_finish(tag, res, rows)
    assert done == ({1, 3} if n <= 5 else {1, 3, 63} if n == 64 else {1, 255} if Nx == 700 else {1, 3, 63, 255, 999})


def other_cases():
    sig = lambda m: 0.05 + 0.2 * np.abs(np.sin(np.arange(m)))       # noqa: E731  (tests/test_parity_gpu.py::test_chi_square_likelihood)
    c1, c2 = synth.workload_c1(Nx=700), synth.workload_c2(Nx=257)
    return {
        "id11-p1": (c1, {}), "id11-p3": (c1, dict(p=3.0)), "id11-chi-square": (c1, dict(like=1, sigma=sig(700))),
        "id2-p3": (c2, dict(p=3.0)), "id2-chi-square": (c2, dict(like=1, sigma=sig(257))),
    }


@pytest.mark.parametrize("name", ["id11-p1", "id11-p3", "id11-chi-square", "id2-p3", "id2-chi-square"])
def test_other_paths(accel_mod, name):
    """Cases 1 and 2 on the local model of the fused one-tile launch (id 11), likelihood_p = 3 and chi_square (l without the
    factor 1/2), 100 samples at L = 31 and L = 3."""
    w, kw = other_cases()[name]
    P = synth.chain_params(w, 100)
    y = spectrum_for(w)
    like, p, sigma = kw.get("like", 0), kw.get("p", 1.0), kw.get("sigma")
    with accel_mod.Accel(w["model_case"], w["plength"], w["x"], y, sigma_y=sigma, likelihood_case=like, likelihood_p=p) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0), name
        for max_lag in (31, 3):
            res = run_ess(acc, [P], max_lag, 7)
            check_acov(name, res, rows, y, like, p, sigma)
            check_finish(name, res, rows)


def nan_rows(P, where):
    Q = np.array(P)
    Q[np.asarray(where), 0] = np.nan
    return Q


def test_invariance(accel_mod):
    """Case 3.  150 samples of 65 bins at L = 15 (one full group of lags) and L = 31 (two): every block size and every split
    of either pass gives the bits of one push in blocks of 64."""
    w, y, P = c2_chain(65, 150)
    n = len(P)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        for L in (15, 31):
            base = run_ess(acc, [P], L, 64)
            assert base["lag"] == L
            check_acov("invariance", base, rows, y)
            check_finish("invariance", base, rows)
            for B in (1, 7, 64, 200, 0):
                assert same_ess(run_ess(acc, [P], L, B), base), ("block_chains", B, L)
            for size in (1, L - 1, L, L + 1, n):
                split = [P[k:k + size] for k in range(0, n, size)]
                r = run_ess(acc, [P], L, 7, ess_pushes=split)
                assert same_ess(r, base), ("ESS pass in pushes of", size, L)
                assert np.array_equal(bits(r["ess_out"][0]), bits(base["fold_out"][0])) and np.array_equal(r["ess_out"][1], base["fold_out"][1])
                if size in (1, L + 1):
                    assert same_ess(run_ess(acc, split, L, 64, ess_pushes=[P[:50], P[50:51], P[51:]]), base), ("fold pass in pushes of", size, L)


@pytest.mark.parametrize("where", ["first", "last", "block-edge", "L-in-a-row", "mixed"])
def test_rejected_samples(accel_mod, where):
    """Case 3, rejected samples: a NaN parameter row does not advance t, so the chain with such rows inserted gives the bits
    of the chain without them, at every block size -- first, last, on both sides of a block edge (blocks of 7 and chunks of
    64), L of them in a row, and all of these together."""
    w, y, P = c2_chain(65, 150)
    L = 15
    bad = P[:1]
    pieces = dict(first=[bad, P], last=[P, bad], **{"block-edge": [P[:6], bad, bad, P[6:62], bad, bad, bad, P[62:]],
                  "L-in-a-row": [P[:40]] + [bad] * L + [P[40:]], "mixed": [bad, P[:6], bad, bad, P[6:40]] + [bad] * L + [P[40:], bad]})[where]
    Q = np.concatenate(pieces)
    isbad = np.concatenate([np.full(len(a), a is bad) for a in pieces])
    Q = nan_rows(Q, np.flatnonzero(isbad))
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        clean = run_ess(acc, [P], L, 64)
        for B in (7, 64, 1, 0):
            r = run_ess(acc, [Q], L, B)
            assert r["n_used"] == len(P) and r["n_rejected"] == int(isbad.sum())
            assert np.array_equal(r["ess_out"][1] != 0, isbad) and np.array_equal(r["ess_out"][1], r["fold_out"][1])
            assert np.array_equal(bits(r["ess_out"][0]), bits(r["fold_out"][0]))
            assert same_ess(r, clean, skip=("n_rejected",)), (where, B)
        split = [Q[k:k + L] for k in range(0, len(Q), L)]
        assert same_ess(run_ess(acc, [Q], L, 7, ess_pushes=split), clean, skip=("n_rejected",)), (where, "pushes of L")


def test_nothing_else_moves(accel_mod):
    """Case 4: the fold, predictive and window results before the ESS pass, during it and after ess_end, byte for byte; and
    fold pushes after ess_end continue as if the mode had never been on."""
    w, y, P = c2_chain(257, 60)
    extra = synth.chain_params(w, 9, seed=4242)

    def snapshot(s):
        return s.result(), s.predictive_result(), s.window_result()

    def same_snapshot(a, b):
        return same(a[0], b[0]) and all(np.array_equal(bits(np.asarray(a[1][k], dtype=np.float64)), bits(np.asarray(b[1][k], dtype=np.float64))) for k in PRED_KEYS) and \
            all(np.array_equal(bits(np.asarray(a[2][k], dtype=np.float64)), bits(np.asarray(b[2][k], dtype=np.float64))) for k in WIN_KEYS)

    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        with capi.Summary(acc, 7, predictive=True, window=(7, 3)) as s, capi.Summary(acc, 7, predictive=True, window=(7, 3)) as never:
            s.push(P)
            before = snapshot(s)
            s.ess_begin(15)
            assert same_snapshot(snapshot(s), before), "entering the mode"
            s.push(P[:31])
            assert same_snapshot(snapshot(s), before), "half a pass"
            s.push(P[31:])
            r = s.ess_result()
            assert r["n_used"] == 60 and same_snapshot(snapshot(s), before), "a whole pass"
            s.ess_end()
            assert same_snapshot(snapshot(s), before), "after ess_end"
            s.push(extra)
            never.push(P)
            never.push(extra)
            assert same_snapshot(snapshot(s), snapshot(never)), "a summary that never entered the mode differs"


def n0_chain(w, series):
    """A chain that moves only the white-noise level, the last noise parameter."""
    k = w["names"].index("White_Noise_N0")
    P = np.tile(w["params_true"], (len(series), 1))
    P[:, k] = w["params_true"][k] + series
    return P


def test_known_answer(accel_mod):
    """Case 5.  M_is = N0_s + c_i, so every bin's series is the N0 series: its ESS is the rule applied in numpy to that
    sequence.  sigma = 0.002 about N0 = 0.134; numpy seed 1 (checked below on the numpy side: every |P_m| up to the cut above
    1e-6 and a stationary R-hat below 1.01)."""
    n, sd, seed = 4000, 0.002, 1
    w = synth.workload_c2(Nx=65)
    y = spectrum_for(w)
    Nx = 65
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        # phi = 0.8 at L = 63
        x = R.ar1(0.8, n, sd, seed)
        tau, ess, cut, Pm = R.ess_of_sequence(x, 63)
        assert np.all(np.abs(Pm[:cut // 2 + 1]) > 1e-6) and cut < 64
        assert float(R.rhat(x[:, None])[0]) < 1.01
        r = run_ess(acc, [n0_chain(w, x)], 63, acov=False)
        assert r["n_used"] == n and r["lag"] == 63
        rel = float(np.max(np.abs(r["ess_M"] - ess) / ess))
        print(f"KNOWN phi=0.8: ess {ess:.6g} (n (1 - phi) / (1 + phi) = {n / 9:.6g}), cut {cut}, max relative difference over the bins {rel:.3g}, "
              f"rhat {float(np.max(r['rhat_M'])):.6g}")
        assert rel <= 1e-6 and np.all(r["cut_M"] == cut)
        assert np.all(r["ess_M"] >= 0.5 * n / 9) and np.all(r["ess_M"] <= 2.0 * n / 9)
        assert np.all(r["rhat_M"] < 1.01) and r["n_rhat_high"] == 0 and r["n_truncated_M"] == 0
        assert np.allclose(r["mcse_M"], sd * np.std(x / sd, ddof=1) / np.sqrt(ess), rtol=1e-6)
        # the same chain shifted by 3 sigma from the middle on
        xs = x.copy()
        xs[n // 2:] += 3.0 * sd
        r = run_ess(acc, [n0_chain(w, xs)], 63, acov=False)
        print(f"KNOWN shifted: rhat {float(np.min(r['rhat_M'])):.6g} ... {float(np.max(r['rhat_M'])):.6g}")
        assert np.all(r["rhat_M"] > 1.5) and r["n_rhat_high"] == Nx and r["bin_max_rhat"] >= 0
        # phi = 0.99 at L = 15: every bin truncated
        x = R.ar1(0.99, n, sd, seed)
        assert R.ess_of_sequence(x, 15)[2] == 16
        r = run_ess(acc, [n0_chain(w, x)], 15, acov=False)
        assert np.all(r["cut_M"] == 16) and r["n_truncated_M"] == Nx
        # phi = -0.5: more than n, and no more than the floor allows
        x = R.ar1(-0.5, n, sd, seed)
        _, ess, cut, Pm = R.ess_of_sequence(x, 63)
        assert np.all(np.abs(Pm[:cut // 2 + 1]) > 1e-6)
        r = run_ess(acc, [n0_chain(w, x)], 63, acov=False)
        print(f"KNOWN phi=-0.5: ess {ess:.6g}, max relative difference {float(np.max(np.abs(r['ess_M'] - ess) / ess)):.3g}")
        assert np.all(r["ess_M"] > n) and np.all(r["ess_M"] <= n * np.log10(n)) and np.all(r["cut_M"] == cut)
        assert float(np.max(np.abs(r["ess_M"] - ess) / ess)) <= 1e-6


def test_refusals_and_state(accel_mod):
    """Case 6."""
    w, y, P = c2_chain(257, 37)
    T = np.ones(len(P))
    E = capi.E_INVALID
    extra = synth.chain_params(w, 5, seed=4242)

    def refused(fn, *a):
        with pytest.raises(accel_mod.AccelError) as e:
            fn(*a)
        assert e.value.code == E

    acc = accel_mod.Accel(2, w["plength"], w["x"], y)
    clean = run_ess(acc, [P], 15)
    s = capi.Summary(acc, 8)
    refused(s.ess_begin)                                                     # before any push: n_used < 4
    refused(s.ess_result)
    refused(s.ess_acov, 0)
    refused(s.ess_end)
    s.push(P[:3])
    refused(s.ess_begin)                                                     # three samples
    s.push(P[3:4])
    assert s.ess_begin() == 3                                                # four: L = 3
    s.ess_end()
    s.push(P[4:])
    full = s.result()
    refused(s.ess_begin, -1)                                                 # max_lag outside 0 ... 1023
    refused(s.ess_begin, 1024)
    s.quantiles_begin((0.16, 0.5, 0.84))
    refused(s.ess_begin)                                                     # in quantile mode
    s.quantiles_end()
    s.loo_begin()
    refused(s.ess_begin)                                                     # in LOO mode
    s.loo_end()
    acc.begin(P, T)                                                          # a batch in flight
    refused(s.ess_begin)
    acc.end()
    acc.arm(len(P))                                                          # a batch armed
    refused(s.ess_begin)
    acc.disarm()
    assert s.ess_begin(1023) == 35                                           # clipped to n - 1 = 36, odd
    s.ess_end()
    assert s.ess_begin(15) == 15
    refused(s.ess_begin)                                                     # twice in a row
    refused(s.quantiles_begin, (0.5,))                                       # the other modes are refused in ESS mode
    refused(s.loo_begin)
    refused(s.predictive_enable)
    refused(s.window_enable, 7)
    refused(s.ess_result)                                                    # nothing pushed
    refused(s.ess_acov, 0)
    s.push(P[:-1])                                                           # a pass with one sample missing
    refused(s.ess_acov, 1)
    refused(s.ess_result)
    s.push(P)
    s.push(P[3:4])                                                           # one sample too many
    refused(s.ess_result)
    s.push(P[:20])                                                           # the full pass, in two pushes
    s.push(P[20:])
    refused(s.ess_acov, 2)
    refused(s.ess_acov, -1)
    r = s.ess_result()
    r["acov_M"], r["acov_l"] = s.ess_acov(0), s.ess_acov(1)
    assert same_ess(r, clean), "after discarded passes"
    assert same_ess(s.ess_result(), clean), "a second result without another pass"
    assert same(s.result(), full)
    s.ess_end()
    refused(s.ess_result)
    refused(s.ess_acov, 0)
    refused(s.ess_end)
    s.push(extra)                                                            # folds on as if nothing had happened
    after = s.result()
    with capi.Summary(acc, 8) as s2:
        s2.push(P)
        s2.push(extra)
        assert same(s2.result(), after), "a summary that never entered the mode differs"
    d = s.ess(np.concatenate([P, extra]), 7)                                 # the convenience call leaves the mode
    assert d["n_used"] == len(P) + 5 and d["lag"] == 7
    refused(s.ess_end)
    s.ess_begin()
    s.push(P[:9])
    s.reset()                                                                # leaves the mode, forgets every sample
    refused(s.ess_result)
    assert s.result()["n_used"] == 0
    s.push(P)
    assert same(s.result(), full)
    s.loo_begin()                                                            # the other modes work after it
    s.loo_end()
    s.ess_begin()
    s.push(P[:9])
    refused(acc.close)                                                       # a live summary holds the context
    s.close()                                                                # inside the mode, a pass half pushed
    acc.close()


def test_at_length(accel_mod):
    """A real chain's length: 70 001 samples of a 65-bin grid at L = 255 in blocks of 64 and of 131 073 -- 1094 blocks against
    one block cut into 1094 chunks, sample indices past 65 535 -- bit for bit the same; the finish on every bin; the
    long-double lag products on four bins (all 65 would take the reference half a minute)."""
    S = 70001
    w = synth.workload_c2(Nx=65)
    y = spectrum_for(w)
    P = synth.chain_params(w, S)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        a = run_ess(acc, [P], 255, 64)
        b = run_ess(acc, [P], 255, 131073, ess_pushes=[P[:65536], P[65536:65537], P[65537:]])
    assert a["n_used"] == S and a["lag"] == 255 and same_ess(a, b)
    check_finish("at-length", a, rows)
    check_acov("at-length", a, rows, y, sel=[0, 21, 43, 64])
    # an independent chain: tau near 1 in every bin
    assert np.all(a["cut_M"] < 256) and np.all(np.abs(a["tau_M"] - 1.0) < 0.1), (float(a["tau_M"].min()), float(a["tau_M"].max()))


def _device_check():
    """Body of test_device_pointers, in a process where torch owns the device first (as bench.py)."""
    import torch
    import tamcmc_amd as accel_mod
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    w, y, P = c2_chain(65, 150)
    Q = nan_rows(P, [0, 63, 64, 149])
    n = len(Q)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        host = run_ess(acc, [Q], 15, 7)
        assert host["n_rejected"] == 4
        acc.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        dP = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
        dL = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
        dS = torch.full((n,), -9, dtype=torch.int32, device=dev)
        with capi.Summary(acc, 64) as s:
            s.push_device(n, dP.data_ptr())
            assert s.ess_begin(15) == 15
            s.push_device(10, dP.data_ptr(), dL.data_ptr(), dS.data_ptr())   # enqueued, no sync; with and without outputs
            s.push_device(n - 10, dP[10:].data_ptr(), dL[10:].data_ptr(), dS[10:].data_ptr())
            r = s.ess_result()
            r["acov_M"], r["acov_l"] = s.ess_acov(0), s.ess_acov(1)
            assert same_ess(r, host)
            assert np.array_equal(bits(dL.cpu().numpy()), bits(host["fold_out"][0])) and np.array_equal(dS.cpu().numpy(), host["fold_out"][1])
            s.ess_end()
        acc.set_stream(0)
    print("ess device path ok")


def test_device_pointers():
    in_torch_process("test_summary_ess_gpu", "_device_check", "ess device path ok")
