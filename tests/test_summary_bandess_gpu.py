"""ESS and MCSE of the credible-band edges on the GPU (tamcmc_summary_bandess_*, include/tamcmc_accel.h; tamcmc_bandess.hip):
per bin and threshold the indicator series M_t <= thr over the accepted samples in push order, bit-packed on the device, its
lag products as integer counts, the centred products times n^2 in int64, and Geyer's rule on them.

Reference: tests/bandess_reference.py, numpy on the GPU's own rows (eval_batch with every chain in model_rows; the pushes
produce those bits, which the quantile suite relies on too).  The device side is exact, so the comparisons are equalities:

1. Exact: bandess_counts' C_k and E_k equal the reference's integers, count_le equals N, cut is equal, tau and ess are within
   4 ulp of ess_reference.finish on float64(E) (0 expected: the slack is the host's log10, as in the ESS suite), p_hat and
   mcse_p equal their stated expressions bit for bit.  Printed before asserted (pytest -s).
2. Thresholds: the quantile selection's exact values (ties at the threshold included), below min_M, max_M, +inf, NaN, and an
   array that differs wildly from bin to bin.
3. Rejected rows do not advance t: results equal those of the chain without them, bit for bit.
4. Invariance, bit for bit: block_chains, the split of the second pass, host against device pointers.
5. Nothing else moves: fold, predictive, window and scan results, and a quantile selection after the mode.
6. Known answer: a chain that moves only the white-noise level as an AR(1) sequence.
7. The protocol: every refusal, a short pass, mutual exclusion with the other modes, reset and destroy inside the mode.
8. Summary.band_ess equals the step-by-step calls and always leaves the mode.

Worst ulp distance of case 1 and the two ESS values of case 6 observed on an MI355X: see README.md ("Band ESS").
"""
import functools

import numpy as np
import pytest

import bandess_reference as B
import ess_reference as R
from summary_support import Q8, band_pass, c2_chain, gpu_rows, order_stats, ranks_of, same, same_scans, spectrum_for
from support import bits, in_torch_process
from tamcmc_amd import capi, synth

pytestmark = pytest.mark.gpu

PRED_KEYS = capi.Summary.PREDICTIVE_ARRAYS + capi.Summary.PREDICTIVE_TOTALS + ("pit_hist",)
WIN_KEYS = capi.Summary.WINDOW_ARRAYS + capi.Summary.WINDOW_TOTALS + ("pit_hist",)
LEVELS = (0.5, 0.025, 0.975, 0.16, 0.84, 0.3, 1.0, 0.0)    # case 1's thresholds: order statistics of the rows, so `<=` meets equality


def run_band(acc, pushes, thr, max_lag=0, block=0, band_pushes=None, counts=True):
    """Fold pass over `pushes`, band pass over `band_pushes` (default: the same pushes)."""
    with capi.Summary(acc, block) as s:
        out0 = [s.push(P) for P in pushes]
        fold = s.result()
        r = band_pass(s, pushes if band_pushes is None else band_pushes, thr, max_lag, counts)
        assert same(s.result(), fold), "the fold results changed in band ESS mode"
    r["fold"] = fold
    r["fold_out"] = (np.concatenate([a[0] for a in out0]), np.concatenate([a[1] for a in out0]))
    return r


LAGS = (1, 3, 15, 63, 65, 127, 129, 255, 1023)


@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 127, 128, 129, 1100])
@pytest.mark.parametrize("Nx", [2, 63, 64, 65, 257, 700])
def test_exact(accel_mod, Nx, n):
    """Case 1 on id 2, chi(2,2p) with p = 1: a partial wave of bins, one wave less a bin, exactly, and a bin; several workgroups;
    chains that end one short of a word, on it and one past it (63 ... 65, 127 ... 129), and one of 18 chunks; every lag limit
    of the list that n - 1 admits (L = 65 and 129 have a last lag group of 2; 63 and 127 reach back exactly one and two words),
    1023 at 65 bins only; K = 1, 3 and 8 thresholds -- the first K of eight order statistics of the bin's own rows, the
    maximum (a constant series) and the minimum among them.  The fold pass runs once; the reference counts are computed once
    at the largest lag limit, every C_k, H_k, T_k and E_k being the same number at every L."""
    w, y, P = c2_chain(Nx, n)
    lags = [L for L in LAGS if L <= n - 1 and (L != 1023 or Nx == 65)]
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        thr = order_stats(rows, LEVELS)
        ref = B.Counts(rows, thr, max(lags))
        with capi.Summary(acc) as s:
            s.push(P)
            for L in lags:
                for K in (1, 3, 8):
                    res = band_pass(s, [P], thr[:K], L)
                    B.check_exact(f"Nx={Nx} n={n}", res, ref, L)
                    assert res["n_constant"][6 if K == 8 else 0] == (Nx if K == 8 else 0)


@pytest.mark.parametrize("name", ["id11", "chi-square"])
def test_other_paths(accel_mod, name):
    """Case 1 on the local model of the fused one-tile launch (id 11) and under chi_square: the series does not depend on the
    likelihood; this guards the row walk.  100 samples at L = 31 and 3, blocks of 7."""
    w = synth.workload_c1(Nx=700) if name == "id11" else synth.workload_c2(Nx=257)
    P = synth.chain_params(w, 100)
    y = spectrum_for(w)
    kw = {} if name == "id11" else dict(sigma_y=0.05 + 0.2 * np.abs(np.sin(np.arange(257))), likelihood_case=1)
    with accel_mod.Accel(w["model_case"], w["plength"], w["x"], y, **kw) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0), name
        thr = order_stats(rows, LEVELS[:3])
        ref = B.Counts(rows, thr, 31)
        for L in (31, 3):
            B.check_exact(name, run_band(acc, [P], thr, L, 7), ref, L)


def test_thresholds(accel_mod):
    """Case 2.  150 samples of 65 bins, 20 of them duplicates of earlier rows, so that values repeat within a bin."""
    w, y, P0 = c2_chain(65, 130)
    P = np.concatenate([P0, P0[5:25]])
    n, Nx = len(P), 65
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        with capi.Summary(acc, 7) as s:
            s.push(P)
            fold = s.result()
            q = s.quantiles(P, Q8)
            assert q["bits_left"] == 0 and np.array_equal(bits(q["lo"]), bits(q["hi"]))
            # the selection's exact values: at least rank + 1 samples lie at or below each, exactly that many where the value is met once
            res = band_pass(s, [P], q["lo"], 15)
            B.check_exact("selection", res, B.Counts(rows, q["lo"], 15), 15)
            ranks = ranks_of(Q8, n)
            assert np.array_equal(q["ranks"], ranks)
            once = (rows[None, :, :] == q["lo"][:, None, :]).sum(axis=1) == 1
            assert np.all(res["count_le"] >= ranks[:, None] + 1)
            assert np.array_equal(res["count_le"][once], np.broadcast_to(ranks[:, None] + 1, once.shape)[once])
            assert (~once).any() and once.any(), "the duplicated rows give ties at a threshold somewhere, and not everywhere"
            assert np.array_equal(res["count_le"][6], np.full(Nx, n)) and res["n_constant"][6] == Nx          # q = 1: the maximum
            # below min_M, max_M, +inf, NaN, -inf, and an array that differs wildly from bin to bin
            wild = np.where(np.arange(Nx) % 3 == 0, -1e300, np.where(np.arange(Nx) % 3 == 1, fold["mean_M"], 1e300))
            wild[7], wild[8], wild[9] = np.nan, np.inf, -0.0
            thr = np.stack([np.nextafter(fold["min_M"], -np.inf), fold["max_M"], np.full(Nx, np.inf), np.full(Nx, np.nan), np.full(Nx, -np.inf), wild,
                            fold["min_M"]])
            res = band_pass(s, [P], thr, 15)
            B.check_exact("special", res, B.Counts(rows, thr, 15), 15)
            for j, N in ((0, 0), (1, n), (2, n), (3, 0), (4, 0)):
                assert np.all(res["count_le"][j] == N) and np.all(np.isnan(res["ess"][j])) and np.all(np.isnan(res["mcse_p"][j])), j
                assert np.all(res["cut"][j] == 0) and res["n_constant"][j] == Nx and res["bin_min_ess"][j] == -1 and np.isnan(res["min_ess"][j]), j
                assert np.all(res["p_hat"][j] == (1.0 if N else 0.0))
            assert np.all(res["count_le"][6] >= 1) and np.all(res["count_le"][5][0::3] == 0) and np.all(res["count_le"][5][2::3][3:] == n)
            assert res["count_le"][5][7] == 0 and res["count_le"][5][8] == n and res["count_le"][5][9] == 0


def nan_rows(P, where):
    Q = np.array(P)
    Q[np.asarray(where, dtype=np.int64), 0] = np.nan
    return Q


@functools.lru_cache(maxsize=None)
def chain_150():
    """The chain of cases 3, 4 and 8: 150 samples of 65 bins, and three thresholds per bin near its 2.5, 50 and 97.5 % values
    (fixed numbers: a function of the bin, not of the GPU's rows)."""
    w, y, P = c2_chain(65, 150)
    return w, y, P


def thresholds_150(acc, P):
    _, st, rows = gpu_rows(acc, P)
    assert np.all(st == 0)
    return rows, order_stats(rows, (0.025, 0.5, 0.975))


@pytest.mark.parametrize("where", ["first", "last", "0-63-64-65", "run-64", "run-130", "L-in-a-row"])
def test_rejected_rows(accel_mod, where):
    """Case 3.  A NaN parameter row is rejected and does not advance t: the chain with such rows inserted gives the bits of the
    chain without them -- first, last, at pushed positions 0, 63, 64 and 65 (both sides of a chunk's and a word's edge), as a
    run of 64 and of 130 from pushed position 64 on (whole chunks rejected, in blocks of 64), and L in a row."""
    w, y, P = chain_150()
    L = 15
    bad = P[:1]
    pieces = {"first": [bad, P], "last": [P, bad], "0-63-64-65": [bad, P[:62], bad, bad, bad, P[62:]],
              "run-64": [P[:64]] + [bad] * 64 + [P[64:]], "run-130": [P[:64]] + [bad] * 130 + [P[64:]],
              "L-in-a-row": [P[:40]] + [bad] * L + [P[40:]]}[where]
    Q = np.concatenate(pieces)
    isbad = np.concatenate([np.full(len(a), a is bad) for a in pieces])
    Q = nan_rows(Q, np.flatnonzero(isbad))
    if where == "0-63-64-65":
        assert list(np.flatnonzero(isbad)) == [0, 63, 64, 65]
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        rows, thr = thresholds_150(acc, P)
        clean = run_band(acc, [P], thr, L, 64)
        B.check_exact("clean", clean, B.Counts(rows, thr, L), L)
        for blk in (64, 7, 0):
            r = run_band(acc, [Q], thr, L, blk)
            assert r["n_used"] == len(P) and r["n_rejected"] == int(isbad.sum())
            assert np.array_equal(r["band_out"][1] != 0, isbad) and np.array_equal(r["band_out"][1], r["fold_out"][1])
            assert np.array_equal(bits(r["band_out"][0]), bits(r["fold_out"][0]))
            assert B.same_band(r, clean, skip=("n_rejected",)), (where, blk)


def test_invariance(accel_mod):
    """Case 4.  150 samples of 65 bins at L = 15 (one full group of lags) and L = 65 (four and a group of 2; more than a word
    back): every block size and every split of the second pass gives the bits of one push in blocks of 64."""
    w, y, P = chain_150()
    n = len(P)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        rows, thr = thresholds_150(acc, P)
        for L in (15, 65):
            base = run_band(acc, [P], thr, L, 64)
            B.check_exact("invariance", base, B.Counts(rows, thr, L), L)
            for blk in (1, 7, 64, 65, 1000):
                assert B.same_band(run_band(acc, [P], thr, L, blk), base), ("block_chains", blk, L)
            for size in (1, L - 1, 40):
                split = [P[k:k + size] for k in range(0, n, size)]
                r = run_band(acc, [P], thr, L, 7, band_pushes=split)
                assert B.same_band(r, base), ("band pass in pushes of", size, L)
                assert np.array_equal(bits(r["band_out"][0]), bits(base["fold_out"][0])) and np.array_equal(r["band_out"][1], base["fold_out"][1])
            # split differently from the fold pass, both ways
            assert B.same_band(run_band(acc, [P[:50], P[50:51], P[51:]], thr, L, 64, band_pushes=[P[:3], P[3:130], P[130:]]), base), L


def _device_check():
    """Body of test_device_pointers, in a process where torch owns the device first (as bench.py)."""
    import torch
    import tamcmc_amd as accel_mod
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    w, y, P = chain_150()
    Q = nan_rows(P, [0, 63, 64, 149])
    n = len(Q)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, thr = thresholds_150(acc, P)
        host = run_band(acc, [Q], thr, 15, 7)
        assert host["n_rejected"] == 4
        acc.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        dP = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
        dL = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
        dS = torch.full((n,), -9, dtype=torch.int32, device=dev)
        with capi.Summary(acc, 64) as s:
            s.push_device(n, dP.data_ptr())
            assert s.bandess_begin(thr, 15) == 15
            s.push_device(10, dP.data_ptr(), dL.data_ptr(), dS.data_ptr())   # enqueued, no sync
            s.push_device(n - 10, dP[10:].data_ptr(), dL[10:].data_ptr(), dS[10:].data_ptr())
            r = s.bandess_result()
            ce = [s.bandess_counts(j) for j in range(3)]
            r["C"], r["E"] = [a for a, _ in ce], [b for _, b in ce]
            assert B.same_band(r, host)
            assert np.array_equal(bits(dL.cpu().numpy()), bits(host["fold_out"][0])) and np.array_equal(dS.cpu().numpy(), host["fold_out"][1])
            s.bandess_end()
        acc.set_stream(0)
    print("bandess device path ok")


def test_device_pointers():
    in_torch_process("test_summary_bandess_gpu", "_device_check", "bandess device path ok")


def test_nothing_else_moves(accel_mod):
    """Case 5: the fold, predictive, window and scan results before the band pass, during it and after bandess_end, byte for
    byte; fold pushes afterwards continue as if the mode had never been on; and a quantile selection after the mode gives
    the brackets of the one before it."""
    w, y, P = c2_chain(257, 60)
    extra = synth.chain_params(w, 9, seed=4242)

    def snapshot(s):
        return s.result(), s.predictive_result(), s.window_result(), [s.scan_result(k) for k in range(2)]

    def same_snapshot(a, b):
        return same(a[0], b[0]) and all(np.array_equal(bits(np.asarray(a[1][k], dtype=np.float64)), bits(np.asarray(b[1][k], dtype=np.float64))) for k in PRED_KEYS) and \
            all(np.array_equal(bits(np.asarray(a[2][k], dtype=np.float64)), bits(np.asarray(b[2][k], dtype=np.float64))) for k in WIN_KEYS) and \
            same_scans(a[3], b[3])

    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        kw = dict(predictive=True, window=(7, 3), scan=(5, 11))
        with capi.Summary(acc, 7, **kw) as s, capi.Summary(acc, 7, **kw) as never:
            s.push(P)
            before = snapshot(s)
            q0 = s.quantiles(P, (0.025, 0.5, 0.975))
            s.bandess_begin(q0["lo"], 15)
            assert same_snapshot(snapshot(s), before), "entering the mode"
            s.push(P[:31])
            assert same_snapshot(snapshot(s), before), "half a pass"
            s.push(P[31:])
            r = s.bandess_result()
            s.bandess_counts(2)
            assert r["n_used"] == 60 and same_snapshot(snapshot(s), before), "a whole pass"
            s.bandess_end()
            assert same_snapshot(snapshot(s), before), "after bandess_end"
            q1 = s.quantiles(P, (0.025, 0.5, 0.975))
            assert all(np.array_equal(bits(np.asarray(q0[k], dtype=np.float64)), bits(np.asarray(q1[k], dtype=np.float64))) for k in ("lo", "hi", "ranks")) and \
                q0["passes"] == q1["passes"], "the selection after the mode"
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
    """Case 6.  The ESS suite's AR(1) chain (phi = 0.8, 4000 samples, sigma = 0.002 about N0, numpy seed 1) moves only the
    white-noise level, and every bin's model is increasing in that level: at each bin's own median and at its 2.5 % value the
    indicator series of every bin is that of the sequence itself at that quantile -- the same integers C_k and E_k, hence the
    same ESS to the last bit."""
    n, sd, seed, L = 4000, 0.002, 1, 63
    w = synth.workload_c2(Nx=65)
    y = spectrum_for(w)
    x = R.ar1(0.8, n, sd, seed)
    P = n0_chain(w, x)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        with capi.Summary(acc) as s:
            s.push(P)
            mean = s.ess(P, L)
            q = s.quantiles(P, (0.5, 0.025))
            res = band_pass(s, [P], q["lo"], L)
    xs = np.sort(x)
    seq = B.Counts(x[:, None], np.array([[xs[r]] for r in ranks_of((0.5, 0.025), n)]), L)
    for j in range(2):
        N, C, E = seq.per[j]
        assert int(N[0]) == ranks_of((0.5, 0.025), n)[j] + 1
        assert np.array_equal(res["count_le"][j], np.full(65, N[0]))
        assert np.array_equal(res["C"][j], np.repeat(C, 65, axis=1)) and np.array_equal(res["E"][j].astype(object), np.repeat(E, 65, axis=1)), j
        assert len(set(bits(res["ess"][j]).tolist())) == 1 and len(set(bits(res["tau"][j]).tolist())) == 1 and len(set(res["cut"][j].tolist())) == 1
        assert B.ulps(res["ess"][j], np.full(65, seq.finish(j, L)[1][0])) <= 4.0
    print(f"KNOWN bandess phi=0.8 n={n} L={L}: ess of the mean {float(mean['ess_M'][0]):.6g} ({float(mean['ess_M'].min()):.6g} ... "
          f"{float(mean['ess_M'].max()):.6g} over the bins), of the median {float(res['ess'][0][0]):.6g} (cut {int(res['cut'][0][0])}), "
          f"of the 2.5 % edge {float(res['ess'][1][0]):.6g} (cut {int(res['cut'][1][0])}); n (1 - phi) / (1 + phi) = {n / 9:.6g}")
    assert res["n_truncated"][0] == 0 and res["n_constant"][0] == 0


def test_band_ess_convenience(accel_mod):
    """Case 8: Summary.band_ess equals the step-by-step calls, and leaves fold mode on -- also when a push raises."""
    w, y, P = chain_150()
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        with capi.Summary(acc, 7) as s:
            s.push(P)
            fold = s.result()
            qs = (0.975, 0.5, 0.025)
            d = s.band_ess(P, qs, 15)
            q = s.quantiles(P, qs)
            r = band_pass(s, [P], q["lo"], 15, counts=False)
            assert B.same_band(d, r) and all(np.array_equal(bits(np.asarray(d[k], dtype=np.float64)), bits(np.asarray(q[k], dtype=np.float64))) for k in ("lo", "hi", "ranks", "q"))
            assert d["passes"] == q["passes"] and d["bits_left"] == 0 and d["lag"] == 15 and d["n_thresholds"] == 3
            assert np.array_equal(bits(d["tail_ess"]), bits(np.minimum(r["ess"][2], r["ess"][0])))
            d1 = s.band_ess(P, (0.5, 1.0), 15)                          # q = 1: a constant series, NaN, and it propagates
            assert np.all(np.isnan(d1["tail_ess"])) and np.all(np.isnan(d1["ess"][1])) and np.all(np.isfinite(d1["ess"][0]))
            with pytest.raises(ValueError):
                s.band_ess(P[:, :-1], qs)                               # the first push raises, in quantile mode
            s.loo_begin()                                               # fold mode: another mode can begin
            s.loo_end()

            class Boom(Exception):
                pass
            real, calls = s.push, []

            def push_then_raise(rows):
                calls.append(getattr(s, "_band", None))
                if calls[-1]:
                    raise Boom()                                        # the band pass's push
                return real(rows)
            s.push = push_then_raise
            with pytest.raises(Boom):
                s.band_ess(P, qs, 15)
            del s.push
            assert calls[-1] is not None and s._band is None
            s.ess_begin(3)                                              # fold mode again
            s.ess_end()
            assert same(s.result(), fold)


def test_refusals_and_state(accel_mod):
    """Case 7."""
    w, y, P = c2_chain(257, 37)
    T = np.ones(len(P))
    E = capi.E_INVALID
    Nx = 257
    extra = synth.chain_params(w, 5, seed=4242)

    def refused(fn, *a):
        with pytest.raises(accel_mod.AccelError) as e:
            fn(*a)
        assert e.value.code == E

    acc = accel_mod.Accel(2, w["plength"], w["x"], y)
    _, _, rows = gpu_rows(acc, P)
    thr = order_stats(rows, (0.16, 0.5, 0.84))
    clean = run_band(acc, [P], thr, 15)
    lib = capi.load_library()
    s = capi.Summary(acc, 8)
    refused(s.bandess_begin, thr)                                            # before any push: n_used < 4
    refused(s.bandess_result)
    refused(s.bandess_counts, 0)
    refused(s.bandess_end)
    s.push(P[:3])
    refused(s.bandess_begin, thr)                                            # three samples
    s.push(P[3:4])
    assert s.bandess_begin(thr) == 3                                         # four: L = 3
    s.bandess_end()
    s.push(P[4:])
    full = s.result()
    refused(s.bandess_begin, thr, -1)                                        # max_lag outside 0 ... 1023
    refused(s.bandess_begin, thr, 1024)
    refused(s.bandess_begin, np.zeros((9, Nx)))                              # K outside 1 ... 8
    lag = capi.C.c_int32(-5)
    assert lib.tamcmc_summary_bandess_begin(s._s, 0, thr.ctypes.data_as(capi.C.POINTER(capi.C.c_double)), 0, capi.C.byref(lag)) == E
    assert lib.tamcmc_summary_bandess_begin(s._s, 3, None, 0, capi.C.byref(lag)) == E and lag.value == -5       # NULL thresholds
    s.quantiles_begin((0.16, 0.5, 0.84))
    refused(s.bandess_begin, thr)                                            # in quantile mode
    s.quantiles_end()
    s.loo_begin()
    refused(s.bandess_begin, thr)                                            # in LOO mode
    s.loo_end()
    s.ess_begin()
    refused(s.bandess_begin, thr)                                            # in ESS mode
    s.ess_end()
    acc.begin(P, T)                                                          # a batch in flight
    refused(s.bandess_begin, thr)
    acc.end()
    acc.arm(len(P))                                                          # a batch armed
    refused(s.bandess_begin, thr)
    acc.disarm()
    assert s.bandess_begin(thr, 1023) == 35                                  # clipped to n - 1 = 36, odd
    s.bandess_end()
    assert s.bandess_begin(thr[:1]) == 35                                    # K = 1, a (1, Nx) array
    s.bandess_end()
    assert s.bandess_begin(thr[1], 7) == 7                                   # and a bare (Nx,) one
    s.bandess_end()
    assert s.bandess_begin(thr, 15) == 15
    refused(s.bandess_begin, thr)                                            # twice in a row
    refused(s.quantiles_begin, (0.5,))                                       # the other modes are refused in band ESS mode
    refused(s.loo_begin)
    refused(s.ess_begin)
    refused(s.predictive_enable)
    refused(s.window_enable, 7)
    refused(s.scan_enable, (5,))
    refused(s.bandess_result)                                                # nothing pushed
    refused(s.bandess_counts, 0)
    s.push(P[:-1])                                                           # a pass with one sample missing
    refused(s.bandess_counts, 1)
    refused(s.bandess_result)
    s.push(P)
    s.push(P[3:4])                                                           # one sample too many
    refused(s.bandess_result)
    s.push(P[:20])                                                           # the full pass, in two pushes
    s.push(P[20:])
    refused(s.bandess_counts, 3)                                             # j out of range
    refused(s.bandess_counts, -1)

    def whole(s):
        r = s.bandess_result()
        ce = [s.bandess_counts(j) for j in range(3)]
        r["C"], r["E"] = [a for a, _ in ce], [b for _, b in ce]
        return r
    assert B.same_band(whole(s), clean), "after discarded passes"
    assert B.same_band(whole(s), clean), "a second result without another pass"
    assert same(s.result(), full)
    s.bandess_end()
    refused(s.bandess_result)
    refused(s.bandess_counts, 0)
    refused(s.bandess_end)
    s.push(extra)                                                            # folds on as if nothing had happened
    after = s.result()
    with capi.Summary(acc, 8) as s2:
        s2.push(P)
        s2.push(extra)
        assert same(s2.result(), after), "a summary that never entered the mode differs"
    s.bandess_begin(thr)
    s.push(P[:9])
    s.reset()                                                                # leaves the mode, forgets every sample
    refused(s.bandess_result)
    assert s.result()["n_used"] == 0
    s.push(P)
    assert same(s.result(), full)
    s.loo_begin()                                                            # the other modes work after it
    s.loo_end()
    for begin, end in ((lambda: s.quantiles_begin((0.5,)), s.quantiles_end), (s.loo_begin, s.loo_end), (s.ess_begin, s.ess_end)):
        begin()
        refused(s.bandess_begin, thr)                                        # and refuse the mode while they are on
        end()
    s.bandess_begin(thr)
    s.push(P[:9])
    refused(acc.close)                                                       # a live summary holds the context
    s.close()                                                                # inside the mode, a pass half pushed
    acc.close()
