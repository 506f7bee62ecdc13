"""Posterior summaries of a stored chain on the GPU (tamcmc_summary_*, include/tamcmc_accel.h; tamcmc_summary.hip).

Reference: the oracle's model rows (pyoracle.generate_batch(..., want_models=True)) reduced in numpy in long double --
two-pass mean / variance, log-sum-exp with the exact maximum.

The tolerances are derived, not tuned: reference() and check() of tests/summary_support.py, whose docstring states them.
Every check prints its worst ratio to the bound (pytest -s shows them) before it asserts.

Worst ratios observed on an MI355X over all cases below: lppd 6.0e-3 (chi_square, id 2), min_M / max_M 3.3e-3 (id 3,
asymmetry 10), mean_M 1.0e-3, mean_l 1.2e-3, var_l 6.8e-4, var_M 2.2e-4, totals 1.3e-4.
"""
import subprocess

import numpy as np
import pytest

import workloads as W
from summary_support import (ARRAYS, TOTALS, c2_case, check, f12, header_values, other_cases, reference, same, spectrum_for,
                             stored_chain, summarize)
from support import bits, in_torch_process
from tamcmc_amd import capi, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("Nx", [2, 255, 256, 257, 700, 5000])
def test_grid_ends(accel_mod, Nx):
    """One bin per thread, 256 threads per workgroup: grids of one partial workgroup, exactly one, one and a bin, several."""
    w, y, P, ref, bound = c2_case(Nx)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        res, logL, st = summarize(acc, [P])
        for k in (0, 17, 36):
            L1, st1, _ = acc.eval_batch(P, np.ones(len(P)), model_rows=[k])
            assert bits(L1[k]) == bits(logL[k]) and st1[k] == st[k], (Nx, k)
    assert np.array_equal(st, ref["status"]) and ref["n_used"] == 37
    check(f"grid-ends Nx={Nx}", res, ref, bound)


def test_order_invariant(accel_mod):
    """One thread owns a bin and folds sample by sample in push order: the block size and the split into pushes cannot
    change a bit, and reset() forgets everything."""
    w, y, P, ref, bound = c2_case(5000)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        first, logL0, st0 = summarize(acc, [P], 1)
        check("order-invariant B=1", first, ref, bound)
        for B in (7, 36, 37, 64):
            res, logL, st = summarize(acc, [P], B)
            assert same(res, first), ("block_chains", B)
            assert np.array_equal(bits(logL), bits(logL0)) and np.array_equal(st, st0)
        res, logL, st = summarize(acc, [P[:10], P[10:11], P[11:]], 7)
        assert same(res, first) and np.array_equal(bits(logL), bits(logL0)), "three pushes"
        with capi.Summary(acc, 5) as s:
            s.push(synth.chain_params(w, 9, scale=0.9, seed=12345))          # garbage
            r9 = s.result()
            assert r9["n_used"] + r9["n_rejected"] == 9 and r9["n_used"] >= 1
            s.reset()
            assert s.result()["n_used"] == 0
            s.push(P[:20])
            mid = s.result()                                                  # between pushes: the state is not disturbed
            s.push(P[20:])
            assert mid["n_used"] == 20 and same(s.result(), first), "reset, then two pushes with a result in between"


def test_few_samples(accel_mod):
    w, y, P, _, _ = c2_case(5000)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        with capi.Summary(acc) as s:
            r0 = s.result()                                                   # n = 0: everything is NaN
            assert r0["n_used"] == 0 and r0["n_rejected"] == 0
            assert all(np.all(np.isnan(r0[k])) for k in ARRAYS) and all(np.isnan(r0[k]) for k in TOTALS[2:])
        res1, _, _ = summarize(acc, [P[:1]])
        _, _, row = acc.eval_batch(P[:1], np.ones(1), model_rows=[0])
        res2, _, _ = summarize(acc, [P[:2]])
    ref1, b1 = reference(w, y, P[:1])
    check("S=1", res1, ref1, b1)
    assert np.array_equal(bits(res1["mean_M"]), bits(row[0]))                 # the mean of one sample is the sample
    assert np.array_equal(bits(res1["min_M"]), bits(row[0])) and np.array_equal(bits(res1["max_M"]), bits(row[0]))
    assert np.array_equal(bits(res1["lppd"]), bits(res1["mean_l"]))           # log((1/1) exp l) = l
    ref2, b2 = reference(w, y, P[:2])
    check("S=2", res2, ref2, b2)
    assert np.all(np.isfinite(res2["var_M"])) and np.all(np.isfinite(res2["var_l"]))


def test_rejected_samples(accel_mod):
    """A NaN parameter and an empty truncation window (tests/test_parity_gpu.py::test_status_codes_nan_and_empty_window):
    first in a block, last in a block, alone in a block of one -- left out of every bin, counted, statuses as the oracle's."""
    w = W.make(2, Nx=3000)
    b = W.split(w)
    y = spectrum_for(w)
    good = W.perturbed(w, 10, scale=0.002)
    empty = W.perturbed(w, 1, scale=0.002, seed=8)[0]
    empty[b["q"] + 1] = -1.0           # negative trunc_c -> empty window
    nan = W.perturbed(w, 1, scale=0.002, seed=9)[0]
    nan[b["z"] + 9] = np.nan           # NaN white noise -> NaN logL
    # blocks of 4: | empty g0 g1 nan | nan g2 g3 g4 | g5 g6 g7 empty | g8 g9
    order = [empty, good[0], good[1], nan, nan, good[2], good[3], good[4], good[5], good[6], good[7], empty, good[8], good[9]]
    P = np.array(order)
    ref, bound = reference(w, y, P)
    assert list(ref["status"]) == [2, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 2, 0, 0] and ref["n_rejected"] == 4
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        clean, _, _ = summarize(acc, [good], 3)
        for B in (4, 1, 0):                             # B = 1: every rejected sample is alone in its block
            res, logL, st = summarize(acc, [P], B)
            assert np.array_equal(st, ref["status"]) and res["n_rejected"] == 4 and res["n_used"] == 10, B
            assert np.all(np.isnan(logL[st != 0])) and np.all(np.isfinite(logL[st == 0]))
            for k in ARRAYS + TOTALS[2:]:
                assert np.array_equal(bits(res[k]), bits(clean[k])), (B, k)
        only_bad, _, st = summarize(acc, [P[[0, 3]]], 1)
        assert only_bad["n_used"] == 0 and only_bad["n_rejected"] == 2 and np.all(np.isnan(only_bad["mean_M"]))
    check("rejected", res, ref, bound)


@pytest.mark.parametrize("name", ["c1-id11-fused", "id14", "id3-asym10", "p=2", "chi-square-id0", "chi-square-id2"])
def test_other_paths(accel_mod, name):
    w, P, kw = other_cases()[name]
    mid = w["model_case"]
    if P is None:
        P = synth.chain_params(w, 19) if "err" in w else W.perturbed(w, 19, scale=0.003)
    y = spectrum_for(w)
    like, p, sigma = kw.get("like", 0), kw.get("p", 1.0), kw.get("sigma")
    ref, bound = reference(w, y, P, sigma=sigma, like=like, p=p)
    assert ref["n_rejected"] == 0
    with accel_mod.Accel(mid, w["plength"], w["x"], y, sigma_y=sigma, likelihood_case=like, likelihood_p=p) as acc:
        if name == "c1-id11-fused":
            assert acc.geometry()["tiles"] == 1
        res, logL, st = summarize(acc, [P], 8)
        L1, st1, _ = acc.eval_batch(P, np.ones(len(P)), model_rows=[3])
    assert bits(L1[3]) == bits(logL[3]) and np.array_equal(st, ref["status"])
    check(name, res, ref, bound)


def _device_check():
    """Body of test_device_pointers, in a process where torch owns the device first (as bench.py)."""
    import torch
    import tamcmc_amd as accel_mod
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    w, y, P, _, _ = c2_case(5000)
    n = len(P)
    with accel_mod.Accel(2, w["plength"], w["x"], y) as acc:
        host, logL, st = summarize(acc, [P], 7)
        acc.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        dP = torch.from_numpy(np.ascontiguousarray(P)).to(dev)
        dL = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
        dS = torch.full((n,), -9, dtype=torch.int32, device=dev)
        with capi.Summary(acc, 7) as s:
            s.push_device(n, dP.data_ptr(), dL.data_ptr(), dS.data_ptr())      # enqueued behind the tensors' fills, no sync
            res = s.result()
            assert same(res, host)
            assert np.array_equal(bits(dL.cpu().numpy()), bits(logL)) and np.array_equal(dS.cpu().numpy(), st)
            s.reset()
            s.push_device(10, dP.data_ptr())                                   # neither logL nor status wanted
            s.push_device(n - 10, dP[10:].data_ptr(), 0, dS[10:].data_ptr())
            assert same(s.result(), host)
        acc.set_stream(0)
    print("summary device path ok")


def test_device_pointers():
    in_torch_process("test_summary_gpu", "_device_check", "summary device path ok")


def test_refusals_and_lifetime(accel_mod):
    w, y, P, _, _ = c2_case(5000)
    T = np.ones(len(P))
    E = capi.E_INVALID

    def refused(fn, *a):
        with pytest.raises(accel_mod.AccelError) as e:
            fn(*a)
        assert e.value.code == E

    acc = accel_mod.Accel(2, w["plength"], w["x"], y)
    before = acc.eval_batch(P, T)
    s = capi.Summary(acc, 8)
    refused(capi.Summary, acc, -1)
    refused(s.push, np.zeros((0, acc.Nparams)))                                      # Nsamples < 1
    rc = s._lib.tamcmc_summary_push(s._s, 3, acc.Nparams - 1, capi._dptr(np.ascontiguousarray(P)), None, None)
    assert rc == E                                                                   # Nparams mismatch
    s.push(P[:5])
    acc.begin(P, T)                           # a batch in flight
    refused(s.push, P[5:9])
    refused(s.result)
    refused(capi.Summary, acc)
    acc.end()
    acc.arm(len(P))                           # a batch armed
    refused(s.push, P[5:9])
    refused(s.reset)
    acc.disarm()
    s.push(P[5:])
    refused(acc.set_spectra, np.stack([y, y]))               # the running state belongs to the resident spectrum
    refused(acc.close)                                       # a live summary holds the context
    full = s.result()
    s.close()
    s.close()                                                # (idempotent)
    after = acc.eval_batch(P, T)
    assert np.array_equal(bits(after[0]), bits(before[0])) and np.array_equal(after[1], before[1])
    with capi.Summary(acc, 8) as s2:
        s2.push(P)
        assert same(s2.result(), full)
    acc.set_spectra(np.stack([y, 2.0 * y]))                  # several spectra in one context: out of scope
    refused(capi.Summary, acc)
    acc.close()


def test_command_line(accel_mod, tmp_path):
    """chainsummary_hip on a 50-sample chain of slice 1 of the reference's real spectrum, written by the phase driver
    (oracle evaluator, as tests/test_outputs.py): samples 4, 6, ..., 48 -- the table and the header totals are the
    Python Summary's on the same rows, to the 12 printed digits."""
    s, root, v, rows, common, sel = stored_chain(tmp_path)
    assert v.shape == (50, s.Nvars)
    table = str(tmp_path / "summary.txt")
    r = subprocess.run(common + [table] + sel, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with accel_mod.Accel(s.model_case, s.plength, s.x, s.y, sigma_y=s.sigma_y, likelihood_case=s.likelihood_case,
                         likelihood_p=s.likelihood_p) as acc:
        res, _, st = summarize(acc, [rows])
    assert np.all(st == 0)
    t = np.loadtxt(table)
    assert t.shape == (s.Nx, 8)
    cols = [s.x, s.y, res["mean_M"], np.sqrt(res["var_M"]), res["min_M"], res["max_M"], res["lppd"], res["var_l"]]
    for k, c in enumerate(cols):
        assert np.array_equal(t[:, k], f12(c)), k
    head = header_values(line for line in open(table) if line.startswith("#"))
    assert (int(head["n_used"]), int(head["n_rejected"]), int(head["first"]), int(head["last"]), int(head["thin"])) == (23, 0, 4, 48, 2)
    for k in ("lppd_total", "p_waic", "waic"):
        assert head[k] == "%.12g" % res[k], k
    # an Nvars that is not the setup's is refused
    hdr = open(root + ".hdr").read()
    assert f"! Nvars= {s.Nvars}\n" in hdr
    open(root + ".hdr", "w").write(hdr.replace(f"! Nvars= {s.Nvars}\n", f"! Nvars= {s.Nvars + 1}\n"))
    r = subprocess.run(common + [table], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and f"but the setup has {s.Nvars} variables" in r.stderr
