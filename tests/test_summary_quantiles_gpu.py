"""Exact per-bin quantiles of a stored chain on the GPU (tamcmc_summary_quantiles_*, include/tamcmc_accel.h;
tamcmc_quantile.hip): a radix selection on order-preserving keys, a few bits per pass, the caller pushing the same rows
once per pass.

Truth for the exact checks: the GPU's own model rows (eval_batch with every chain in model_rows), sorted per bin in numpy,
rank k = ceil(q n) - 1 clamped to [0, n - 1] (numpy's "inverted_cdf").  Those checks have no tolerance: brackets must
contain the truth after every step and end bitwise equal to it.

Against the oracle (pyoracle.generate_batch(..., want_models=True), sorted per bin in long double): an order statistic is
1-Lipschitz in the sup norm over the samples, so with the project's per-bin model bar EPS = 1e-12 the bound is
|value - ref| <= EPS max_s |M_is|.  The worst ratio is printed before it is asserted (pytest -s).
Worst ratios observed on an MI355X: 8.6e-4 (id 2, 700 bins), 3.3e-3 (id 3, asymmetry 10).
"""
import subprocess

import numpy as np
import pytest

import workloads as W
from summary_support import (EPS, Q8, c2_case, f12, gpu_rows, header_values, other_cases, ranks_of, same, same_traj, select,
                             spectrum_for, stored_chain, truth_of, unresolved_bits)
from support import LD, bits, in_torch_process, pyorc
from tamcmc_amd import capi, synth

pytestmark = pytest.mark.gpu

Q3 = (0.16, 0.5, 0.84)


@pytest.mark.parametrize("nbits", [1, 4, 6, 0])
@pytest.mark.parametrize("Nx", [2, 63, 64, 65, 257, 700])
def test_exact_and_bracketed(accel_mod, Nx, nbits):
    """Histogram workgroups of 64 bins: a partial one, exactly one, one and a bin, several."""
    w, y, P, _, _ = c2_case(Nx)
    extra = synth.chain_params(w, 5, seed=4242)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        truth = truth_of(rows, Q8)
        u0 = unresolved_bits(rows)
        with capi.Summary(acc) as s:
            s.push(P)
            before = s.result()
            traj, ranks = select(s, Q8, nbits, lambda k: s.push(P), truth=truth, u0=u0)
            assert np.array_equal(ranks, ranks_of(Q8, 37))
            assert len(traj) - 1 == -(-u0 // (nbits or 6)), (len(traj) - 1, u0)
            lo, hi = traj[-1]
            assert np.array_equal(bits(lo), bits(truth)) and np.array_equal(bits(hi), bits(truth))
            assert np.array_equal(bits(traj[0][0]), bits(np.tile(before["min_M"], (8, 1))))       # before the first step: the envelope
            assert np.array_equal(bits(traj[0][1]), bits(np.tile(before["max_M"], (8, 1))))
            assert np.array_equal(bits(lo[0]), bits(before["min_M"])) and np.array_equal(bits(lo[6]), bits(before["max_M"]))
            assert np.array_equal(bits(lo[3]), bits(lo[7])) and all(np.array_equal(bits(a[3]), bits(a[7])) for t in traj for a in t)
            assert s.quantiles_step() == 0                                   # nothing left: a no-op
            assert same(s.result(), before), "the fold results changed in quantile mode"
            s.quantiles_end()
            assert same(s.result(), before)
            s.push(extra)                                                    # folds on as if nothing had happened
            after = s.result()
        with capi.Summary(acc) as s:
            s.push(P)
            s.push(extra)
            assert same(s.result(), after), "a summary that never entered the mode differs"


def test_order_and_block_invariant(accel_mod):
    w, y, P, _, _ = c2_case(700)
    splits = [(10, 11), (1, 36), (20, 21), (5, 6)]

    def three(s, k):
        a, b = splits[k % len(splits)]
        for part in (P[:a], P[a:b], P[b:]):
            s.push(part)

    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, _, rows = gpu_rows(acc, P)
        truth = truth_of(rows, Q8)
        first = None
        for B in (1, 7, 36, 37, 64):
            with capi.Summary(acc, B) as s:
                s.push(P)
                traj, _ = select(s, Q8, 6, lambda k: s.push(P), truth=truth)
            first = first or traj
            assert same_traj(traj, first), ("block_chains", B)
        with capi.Summary(acc, 7) as s:
            s.push(P)
            traj, _ = select(s, Q8, 6, lambda k: three(s, k), truth=truth)
        assert same_traj(traj, first), "three pushes, split differently from pass to pass"
        with capi.Summary(acc, 7) as s:                                      # the convenience call: same end
            s.push(P)
            r = s.quantiles(P, Q8, 6)
            assert r["passes"] == len(first) - 1 and r["bits_left"] == 0 and np.array_equal(r["q"], np.array(Q8))
            assert np.array_equal(bits(r["lo"]), bits(first[-1][0])) and np.array_equal(bits(r["hi"]), bits(first[-1][1]))
            r2 = s.quantiles(P, Q3, 6, max_passes=2)                         # the mode was left, and is left again
            assert r2["passes"] == 2 and r2["bits_left"] > 0
            t3 = truth_of(rows, Q3)
            assert np.all(r2["lo"] <= t3) and np.all(t3 <= r2["hi"]) and np.any(r2["lo"] < r2["hi"])
            with pytest.raises(accel_mod.AccelError):
                s.quantiles_step()


def test_few_and_equal_samples(accel_mod):
    w, y, P, _, _ = c2_case(257)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, _, rows = gpu_rows(acc, P)
        with capi.Summary(acc) as s:                                         # S = 1: resolved before any step
            s.push(P[:1])
            s.quantiles_begin(Q3)
            assert s.quantiles_step() == 0
            r = s.quantiles_result()
            assert np.array_equal(r["ranks"], [0, 0, 0])
            for a in (r["lo"], r["hi"]):
                assert np.array_equal(bits(a), bits(np.tile(rows[0], (3, 1))))
            s.quantiles_end()
            r = s.quantiles(P[:1], Q3)
            assert r["passes"] == 0 and r["bits_left"] == 0 and np.array_equal(bits(r["lo"]), bits(np.tile(rows[0], (3, 1))))
        with capi.Summary(acc) as s:                                         # S = 2
            s.push(P[:2])
            r = s.quantiles(P[:2], (0.0, 0.5, 0.51, 1.0))
            t = truth_of(rows[:2], (0.0, 0.5, 0.51, 1.0))
            assert np.array_equal(r["ranks"], [0, 0, 1, 1]) and r["bits_left"] == 0
            assert np.array_equal(bits(r["lo"]), bits(t)) and np.array_equal(bits(r["hi"]), bits(t))
        with capi.Summary(acc, 300) as s:                                    # 300 copies of one row in one block of 300
            P300 = np.tile(P[5], (300, 1))
            s.push(P300)
            s.quantiles_begin(Q3)
            s.push(P300)                                                     # (counted, nothing to resolve)
            assert s.quantiles_step() == 0
            r = s.quantiles_result()
            assert np.array_equal(r["ranks"], ranks_of(Q3, 300))
            assert np.array_equal(bits(r["lo"]), bits(np.tile(rows[5], (3, 1)))) and np.array_equal(bits(r["hi"]), bits(r["lo"]))
        # 300 samples in one block of 300 that are NOT all equal: two values, 299 copies of one -- one cell of the
        # workgroup's counters takes 299 counts in one launch
        with capi.Summary(acc, 300) as s:
            Pm = np.tile(P[5], (300, 1))
            Pm[123] = P[6]
            s.push(Pm)
            r = s.quantiles(Pm, Q3, 6)
            t = truth_of(np.concatenate([np.tile(rows[5], (299, 1)), rows[6:7]]), Q3)
            assert r["bits_left"] == 0 and np.array_equal(bits(r["lo"]), bits(t)) and np.array_equal(bits(r["hi"]), bits(t))
        with capi.Summary(acc, 16) as s:                                     # every row three times: ties at every rank
            P3 = np.repeat(P, 3, axis=0)
            s.push(P3)
            r = s.quantiles(P3, Q8, 4)
            t = truth_of(np.repeat(rows, 3, axis=0), Q8)
            assert np.array_equal(r["ranks"], ranks_of(Q8, 111)) and r["bits_left"] == 0
            assert np.array_equal(bits(r["lo"]), bits(t)) and np.array_equal(bits(r["hi"]), bits(t))


def rejected_mix():
    """The 14-row mix of tests/test_summary_gpu.py::test_rejected_samples."""
    w = W.make(2, Nx=3000)
    b = W.split(w)
    y = spectrum_for(w)
    good = W.perturbed(w, 10, scale=0.002)
    empty = W.perturbed(w, 1, scale=0.002, seed=8)[0]
    empty[b["q"] + 1] = -1.0
    nan = W.perturbed(w, 1, scale=0.002, seed=9)[0]
    nan[b["z"] + 9] = np.nan
    order = [empty, good[0], good[1], nan, nan, good[2], good[3], good[4], good[5], good[6], good[7], empty, good[8], good[9]]
    return w, y, good, np.array(order)


def test_rejected_samples(accel_mod):
    w, y, good, P = rejected_mix()
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, stg, rows = gpu_rows(acc, good)
        assert np.all(stg == 0)
        truth = truth_of(rows, Q8)
        with capi.Summary(acc, 3) as s:
            s.push(good)
            clean = s.quantiles(good, Q8)
        assert np.array_equal(bits(clean["lo"]), bits(truth)) and clean["bits_left"] == 0
        for B in (4, 1):
            with capi.Summary(acc, B) as s:
                L0, st0 = s.push(P)
                assert list(st0) == [2, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 2, 0, 0]
                s.quantiles_begin(Q8, 6)
                left = None
                while left != 0:
                    L, st = s.push(P)                                        # the same logL / status bits as in fold mode
                    assert np.array_equal(bits(L), bits(L0)) and np.array_equal(st, st0), B
                    left = s.quantiles_step()
                r = s.quantiles_result()
                assert np.array_equal(r["ranks"], clean["ranks"])
                assert np.array_equal(bits(r["lo"]), bits(clean["lo"])) and np.array_equal(bits(r["hi"]), bits(clean["hi"])), B
                tot = s.result()
                assert tot["n_used"] == 10 and tot["n_rejected"] == 4
        with capi.Summary(acc, 1) as s:                                      # nothing accepted: no quantiles
            s.push(P[[0, 3]])
            with pytest.raises(accel_mod.AccelError) as e:
                s.quantiles_begin(Q3)
            assert e.value.code == capi.E_INVALID


def test_consistency_errors(accel_mod):
    w, y, P, _, _ = c2_case(700)
    E = capi.E_INVALID

    def refused(fn, *a):
        with pytest.raises(accel_mod.AccelError) as e:
            fn(*a)
        assert e.value.code == E

    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        _, _, rows = gpu_rows(acc, P)
        truth = truth_of(rows, Q3)
        # right counts, one value outside the envelope: the row that holds bin 0's maximum, with three times its white noise
        swapped = P.copy()
        top = int(np.argmax(rows[:, 0]))
        swapped[top, W.split(w)["z"] + 9] *= 3.0
        _, sts, srow = gpu_rows(acc, swapped)
        assert np.all(sts == 0) and srow[top, 0] > rows[:, 0].max()
        scaled = synth.chain_params(w, 37, scale=0.9, seed=12345)
        _, stc, crow = gpu_rows(acc, scaled)                                 # 37 accepted samples, values outside the envelope
        assert np.all(stc == 0) and np.any((crow < rows.min(axis=0)) | (crow > rows.max(axis=0)))
        with capi.Summary(acc, 8) as s:
            s.push(P)
            s.quantiles_begin(Q3, 6)
            s.push(P)
            assert s.quantiles_step() > 0
            s.push(P)
            assert s.quantiles_step() > 0
            good = s.quantiles_result()
            bad_passes = [lambda: s.push(P[:-1]),                                         # one sample missing
                          lambda: (s.push(P), s.push(P[3:4])),                            # one extra good sample
                          lambda: s.push(scaled),                                         # other rows: right counts, outside the envelope
                          lambda: s.push(swapped),                                        # one row of 37 outside, in one push of many blocks
                          lambda: None]                                                   # nothing pushed
            for k, bad in enumerate(bad_passes):
                bad()
                refused(s.quantiles_step)
                r = s.quantiles_result()
                assert np.array_equal(bits(r["lo"]), bits(good["lo"])) and np.array_equal(bits(r["hi"]), bits(good["hi"])), k
            left = None
            while left != 0:                                                 # correct passes afterwards: the exact result
                s.push(P)
                left = s.quantiles_step()
            r = s.quantiles_result()
            assert np.array_equal(bits(r["lo"]), bits(truth)) and np.array_equal(bits(r["hi"]), bits(truth))


def test_refusals_and_lifetime(accel_mod):
    w, y, P, _, _ = c2_case(257)
    T = np.ones(len(P))
    E = capi.E_INVALID

    def refused(fn, *a):
        with pytest.raises(accel_mod.AccelError) as e:
            fn(*a)
        assert e.value.code == E

    acc = accel_mod.Accel(2, w["plength"], w["x"], y)
    s = capi.Summary(acc, 8)
    refused(s.quantiles_begin, Q3)                                           # before any push: n_used < 1
    refused(s.quantiles_step)
    refused(s.quantiles_result)
    refused(s.quantiles_end)
    s.push(P)
    full = s.result()
    refused(s.quantiles_begin, [])                                           # Nq = 0
    refused(s.quantiles_begin, np.linspace(0.1, 0.9, 9))                     # Nq = 9
    for bad in (-0.1, 1.1, np.nan):
        refused(s.quantiles_begin, [0.5, bad])
    refused(s.quantiles_begin, Q3, -1)
    refused(s.quantiles_begin, Q3, 7)
    assert s._lib.tamcmc_summary_quantiles_begin(s._s, 3, None, 0) == E
    acc.begin(P, T)                                                          # a batch in flight
    refused(s.quantiles_begin, Q3)
    acc.end()
    acc.arm(len(P))                                                          # a batch armed
    refused(s.quantiles_begin, Q3)
    acc.disarm()
    refused(s.quantiles_step)                                                # still outside the mode
    s.quantiles_begin(Q3)
    refused(s.quantiles_begin, Q3)                                           # twice
    acc.begin(P, T)
    refused(s.quantiles_step)
    refused(s.quantiles_result)
    refused(s.quantiles_end)
    acc.end()
    s.push(P)
    assert s.quantiles_step() > 0
    s.reset()                                                                # leaves the mode, forgets every sample
    refused(s.quantiles_step)
    refused(s.quantiles_result)
    refused(s.quantiles_end)
    assert s.result()["n_used"] == 0
    s.push(P)
    assert same(s.result(), full)
    s.quantiles_begin(Q3, 4)
    s.push(P[:9])
    refused(acc.close)                                                       # a live summary holds the context
    s.close()                                                                # inside the mode, a pass half pushed
    s.close()
    acc.close()


def test_other_paths(accel_mod):
    """The fused one-tile launch (id 11), id 3 with asymmetry 10, chi_square on id 2: one triple each, exact."""
    cases = other_cases()
    for name in ("c1-id11-fused", "id3-asym10", "chi-square-id2"):
        w, P, kw = cases[name]
        if P is None:
            P = synth.chain_params(w, 19) if "err" in w else W.perturbed(w, 19, scale=0.003)
        y = spectrum_for(w)
        like, sigma = kw.get("like", 0), kw.get("sigma")
        with accel_mod.Accel(w["model_case"], w["plength"], w["x"], y, sigma_y=sigma, likelihood_case=like) as acc:
            if name == "c1-id11-fused":
                assert acc.geometry()["tiles"] == 1
            _, st, rows = gpu_rows(acc, P)
            assert np.all(st == 0), name
            with capi.Summary(acc, 8) as s:
                s.push(P)
                r = s.quantiles(P, Q3)
        t = truth_of(rows, Q3)
        assert r["bits_left"] == 0 and np.array_equal(bits(r["lo"]), bits(t)) and np.array_equal(bits(r["hi"]), bits(t)), name


def test_negative_model_values(accel_mod):
    """Id 0 (Gaussian + constant: the one model whose amplitude and constant do not pass through abs(), as
    tests/datacases.py::negative_model_case) under chi_square, where a negative model value is an ordinary sample: half the
    rows get a negative constant, so far from the peak a bin's samples straddle zero and keys of both signs occur."""
    w = W.make_gauss(0, Nx=3000)
    sigma = 0.05 + 0.2 * np.abs(np.sin(np.arange(3000)))
    y = spectrum_for(w)
    P = W.perturbed(w, 19, scale=0.003)
    P[::2, 3] = -np.abs(P[::2, 3])
    with accel_mod.Accel(0, w["plength"], w["x"], y, sigma_y=sigma, likelihood_case=1) as acc:
        _, st, rows = gpu_rows(acc, P)
        assert np.all(st == 0)
        straddle = (rows.min(axis=0) < 0) & (rows.max(axis=0) > 0)
        assert straddle.sum() > 100 and not np.all(straddle), "the construction gives no bin with samples of both signs"
        with capi.Summary(acc, 8) as s:
            s.push(P)
            traj, _ = select(s, Q8, 6, lambda k: s.push(P), truth=truth_of(rows, Q8), u0=unresolved_bits(rows))
    t = truth_of(rows, Q8)
    assert np.any(t[2] < 0) and np.any(t[4] > 0)
    assert np.array_equal(bits(traj[-1][0]), bits(t)) and np.array_equal(bits(traj[-1][1]), bits(t))


@pytest.mark.parametrize("name", ["c2-700", "id3-asym10"])
def test_against_the_oracle(accel_mod, name):
    if name == "c2-700":
        w, y, P, _, _ = c2_case(700)
    else:
        w, P, _ = other_cases()[name]
        P = synth.chain_params(w, 19)
        y = spectrum_for(w)
    mid = w["model_case"]
    _, rst, M = pyorc().generate_batch(mid, w["plength"], w["x"], y, P, np.ones(len(P)), want_models=True)
    assert np.all(rst == 0)
    Mq = np.sort(M.astype(LD), axis=0)
    ref = Mq[ranks_of(Q8, len(P))]
    bound = EPS * np.abs(Mq).max(axis=0)
    with accel_mod.Accel(mid, w["plength"], w["x"], y) as acc:
        with capi.Summary(acc) as s:
            s.push(P)
            r = s.quantiles(P, Q8)
    assert r["bits_left"] == 0 and np.array_equal(bits(r["lo"]), bits(r["hi"]))
    ratio = float(np.max(np.abs(r["lo"].astype(LD) - ref) / bound))
    print(f"RATIO quantiles {name}: {ratio:.3g}")
    assert ratio <= 1.0, (name, ratio)


def _device_check():
    """Body of test_device_pointers, in a process where torch owns the device first (as bench.py)."""
    import torch
    import tamcmc_amd as accel_mod
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    w, y, P, _, _ = c2_case(700)
    n = len(P)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        with capi.Summary(acc, 7) as s:
            L0, st0 = s.push(P)
            host = s.quantiles(P, Q8, 4)
        acc.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        dP = torch.from_numpy(np.ascontiguousarray(P)).to(dev)
        dL = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
        dS = torch.full((n,), -9, dtype=torch.int32, device=dev)
        with capi.Summary(acc, 7) as s:
            s.push_device(n, dP.data_ptr())
            s.quantiles_begin(Q8, 4)
            left, passes = None, 0
            while left != 0:
                if passes % 2:                                               # enqueued, no sync; with and without outputs, split or not
                    s.push_device(10, dP.data_ptr())
                    s.push_device(n - 10, dP[10:].data_ptr(), 0, dS[10:].data_ptr())
                else:
                    s.push_device(n, dP.data_ptr(), dL.data_ptr(), dS.data_ptr())
                left = s.quantiles_step()
                passes += 1
            r = s.quantiles_result()
            assert passes == host["passes"]
            assert np.array_equal(bits(r["lo"]), bits(host["lo"])) and np.array_equal(bits(r["hi"]), bits(host["hi"]))
            assert np.array_equal(bits(dL.cpu().numpy()), bits(L0)) and np.array_equal(dS.cpu().numpy(), st0)
            s.quantiles_end()
        acc.set_stream(0)
    print("quantile device path ok")


def test_device_pointers():
    in_torch_process("test_summary_quantiles_gpu", "_device_check", "quantile device path ok")


def test_command_line(accel_mod, tmp_path):
    """The 23-sample chain of summary_support.stored_chain with --quantiles: three more columns, the first eight unchanged,
    the header says which quantiles and how many passes."""
    s, root, v, rows, common, sel = stored_chain(tmp_path)
    plain, table = str(tmp_path / "plain.txt"), str(tmp_path / "bands.txt")
    r = subprocess.run(common + [plain] + sel, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run(common + [table] + sel + ["--quantiles", "0.16,0.5,0.84"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with accel_mod.Accel(s.model_case, s.plength, s.x, s.y, sigma_y=s.sigma_y, likelihood_case=s.likelihood_case,
                         likelihood_p=s.likelihood_p) as acc:
        with capi.Summary(acc) as sm:
            _, st = sm.push(rows)
            q = sm.quantiles(rows, Q3)
    assert np.all(st == 0) and q["bits_left"] == 0
    t0, t = np.loadtxt(plain), np.loadtxt(table)
    assert t0.shape == (s.Nx, 8) and t.shape == (s.Nx, 11)
    assert np.array_equal(t[:, :8], t0)
    for j in range(3):
        assert np.array_equal(t[:, 8 + j], f12(q["lo"][j])), j
    assert np.all(t[:, 4] <= t[:, 8]) and np.all(t[:, 8] <= t[:, 9]) and np.all(t[:, 9] <= t[:, 10]) and np.all(t[:, 10] <= t[:, 5])
    lines0 = [l for l in open(plain) if l.startswith("#")]
    lines = [l for l in open(table) if l.startswith("#")]
    head = header_values(lines)
    assert head["quantiles"] == "0.16,0.5,0.84" and int(head["passes"]) == q["passes"] and int(head["n_used"]) == 23
    assert lines[-1].split() == "# x y mean_M sd_M min_M max_M lppd var_l q0.16 q0.5 q0.84".split()
    assert not any("quantiles=" in l for l in lines0) and lines0[-1].split() == "# x y mean_M sd_M min_M max_M lppd var_l".split()
    assert len(lines) == len(lines0) + 1
