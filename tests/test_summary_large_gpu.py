"""Posterior summaries and quantiles of a chain of real length: N = 70 001 samples (one full run of 65 535 of the
histogram kernel plus a partial one; odd, no multiple of any unroll), blocks longer than a run, and 16-bit counters at
their limit (tamcmc_summary.hip, tamcmc_quantile.hip).  The other summary tests push 37 samples: there the flush loop of
the histogram kernel runs once, no counter passes 37, and the accumulation term n 2^-52 of the bounds never binds.

Case of every test: synth.workload_c2(Nx=65) -- one full histogram wave plus one bin -- id 2, rows = params_true +
0.5 err normal on the variables (numpy.random.default_rng).  The oracle rejects none of them and every model value is
positive.  A block of B samples is one launch over B chains, so blocks of 65 535 ... 131 073 are also the one-tile eval
launch at those chain counts.

Bounds (none is new):
  a. the fold against the oracle: reference() / check() of tests/summary_support.py as they are, E = EPS + n 2^-52 with
     n 2^-52 = 1.6e-11 now the larger term.
  b. accumulation alone: the GPU's own model rows reduced in long double by the same formulas, EPS replaced by 0, so that
     only the n 2^-52 terms remain: |d mean_M| <= acc mean|M|, |d var_M| <= 4 acc mean(M^2), min_M / max_M bit-equal,
     delta = dl + acc max|l| for mean_l / lppd, 2 delta sd_l + delta^2 for var_l.  dl is the rounding of l itself, which
     the kernel computes in fp64 from the same M that the reference takes to long double:
       chi(2,2p)   l = -p (y / M + log M): the quotient (2^-53 y/M), the device log (1 ulp: 2^-52 |log M|), the sum and the
                   product by p (2^-53 (y/M + |log M|) each)           =>  dl <= 2 * 2^-52 p (y/M + |log M|)
       chi_square  l = -((y - M)^2 (1 / sigma^2)): five roundings on the way (difference, counted twice in the square; the
                   square; sigma^2 and its reciprocal on the host; the product), 2^-53 relative each
                                                                       =>  dl <= 3 * 2^-52 |l|
Worst ratios to these bounds observed on an MI355X (pytest -s prints them):
  a. chi(2,2p):  mean_M 9.1e-4, min_M 5.2e-4, max_M 3.6e-4, mean_l 1.0e-3, lppd 1.4e-3, var_M 3.1e-8, var_l 1.3e-5, totals 2.2e-5
     chi_square: mean_l 1.2e-3, lppd 4.3e-2, var_l 2.4e-5, totals 2.2e-6 (the model's own as above)
  b. chi(2,2p):  mean_M 9.7e-4, mean_l 1.1e-3, lppd 5.3e-3, var_M 3.2e-8, var_l 6.8e-5, totals 3.1e-5
     chi_square: mean_l 1.4e-3, lppd 1.0e-1, var_l 3.7e-5, totals 1.1e-6
A fold that counts n in 16 bits fails (a) with NaN means while every 37-sample test passes; TM_Q_RUN = 65536 fails (ii) and
(iii) of the counter cases.  (A fold that divides by (float) n would pass: a float holds every n up to 2^24.)

Quantiles at 1 bit per pass need 50 passes: the block of 70 001 runs them all, to the exact end; the comparison with
block_chains = 64 (1094 launches per pass) covers the first 6 passes there and the whole trajectory at 6 bits.
"""
import functools

import numpy as np
import pytest

import workloads as W
from summary_support import (Q8, accumulation_reference, check, gpu_rows, ranks_of, reference, rows_around, same, same_traj, select, sigma_of, spectrum_for,
                             steps, summarize, truth_of, unresolved_bits)
from support import bits
from tamcmc_amd import capi, synth

pytestmark = pytest.mark.gpu

N = 70001
RUN = 65535                                              # TM_Q_RUN, tamcmc_quantile.h
Q5 = (0.0, 0.16, 0.5, 0.84, 1.0)
ULP = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def case():
    w = synth.workload_c2(Nx=65)
    y = spectrum_for(w)
    P = rows_around(w, N)
    for a in (y, P):
        a.setflags(write=False)
    return w, y, P


@functools.lru_cache(maxsize=None)
def oracle_reference(like):
    w, y, P = case()
    return reference(w, y, P, sigma=sigma_of(65) if like else None, like=like)


def open_case(accel_mod, like=0):
    w, y, _ = case()
    return accel_mod.Accel(2, w["plength"], w["x"], y, sigma_y=sigma_of(65) if like else None, likelihood_case=like)


_ROWS = {}


def rows_of_case(acc, like):
    """The GPU's own rows of the N samples (and logL, status), in batches of 4096 chains; computed once per likelihood."""
    if like not in _ROWS:
        _, _, P = case()
        out = [gpu_rows(acc, P[k:k + 4096]) for k in range(0, N, 4096)]
        _ROWS[like] = tuple(np.concatenate([o[j] for o in out]) for j in range(3))
        for a in _ROWS[like]:
            a.setflags(write=False)
    return _ROWS[like]


@pytest.mark.parametrize("like", [0, 1], ids=["chi22p", "chi-square"])
def test_fold_against_the_oracle(accel_mod, like):
    """1094 launches of the default block of 64; reference() and check() as they are."""
    _, _, P = case()
    ref, bound = oracle_reference(like)
    assert ref["n_used"] == N and ref["n_rejected"] == 0
    with open_case(accel_mod, like) as acc:
        res, logL, st = summarize(acc, [P])
    assert np.array_equal(st, ref["status"])
    assert np.max(np.abs(logL - ref["logL"]) / np.abs(ref["logL"])) <= 1e-10
    check(f"n={N} fold vs oracle like={like}", res, ref, bound)


@pytest.mark.parametrize("like", [0, 1], ids=["chi22p", "chi-square"])
def test_accumulation_alone(accel_mod, like):
    _, y, P = case()
    with open_case(accel_mod, like) as acc:
        _, st, rows = rows_of_case(acc, like)
        assert np.all(st == 0) and np.all(rows > 0)
        res, _, st2 = summarize(acc, [P])
    assert np.array_equal(st2, st)
    ref, bound = accumulation_reference(rows, y, sigma_of(65) if like else None, like)
    assert np.array_equal(bits(res["min_M"]), bits(rows.min(axis=0))) and np.array_equal(bits(res["max_M"]), bits(rows.max(axis=0)))
    check(f"n={N} accumulation alone like={like}", res, ref, bound)


def test_block_size_cannot_change_a_bit(accel_mod):
    _, _, P = case()
    with open_case(accel_mod) as acc:
        first, logL0, st0 = summarize(acc, [P], 64)
        assert first["n_used"] == N
        for B in (64, RUN, RUN + 1, N):
            for pushes in ([P], [P[:1], P[1:RUN + 1], P[RUN + 1:]]):
                if B == 64 and len(pushes) == 1:
                    continue
                res, logL, st = summarize(acc, pushes, B)
                assert same(res, first), ("block_chains", B, len(pushes))
                assert np.array_equal(bits(logL), bits(logL0)) and np.array_equal(st, st0), ("block_chains", B, len(pushes))


@pytest.mark.parametrize("nbits", [1, 6])
def test_quantiles_with_a_block_longer_than_a_run(accel_mod, nbits):
    _, _, P = case()
    with open_case(accel_mod) as acc:
        _, st, rows = rows_of_case(acc, 0)
        truth = truth_of(rows, Q8)
        u0 = unresolved_bits(rows)
        assert u0 >= 45, u0                                                   # 50 here: many passes at either width
        with capi.Summary(acc, N) as s:
            s.push(P)
            traj, ranks = select(s, Q8, nbits, lambda k: s.push(P), truth=truth, u0=u0)
        assert np.array_equal(ranks, ranks_of(Q8, N)) and len(traj) - 1 == -(-u0 // nbits)
        assert np.array_equal(bits(traj[-1][0]), bits(truth)) and np.array_equal(bits(traj[-1][1]), bits(truth))
        with capi.Summary(acc, 64) as s:
            s.push(P)
            if nbits == 6:
                small, _ = select(s, Q8, nbits, lambda k: s.push(P), truth=truth, u0=u0)
            else:
                small = steps(s, Q8, nbits, lambda k: s.push(P), truth, 6)
        assert same_traj(traj[:len(small)], small), "block_chains = 64 narrows differently"


def counter_sequences():
    """Push orders over the rows (A, B, C, NaN) = (0, 1, 2, 3); a block is the whole push."""
    A, B, C = [0], [1], [2]
    three = A * (RUN + 2) + B * RUN + C
    five = np.array(three)
    five[999::1000] = 3
    return {"i": A * RUN + B + C, "ii": A * (RUN + 1) + B + C, "iii": three, "iv": B + A * (2 * RUN) + C, "v": list(five)}


@pytest.mark.parametrize("name", ["i", "ii", "iii", "iv", "v"])
def test_counters_at_their_limit(accel_mod, name):
    """One value 65 535, 65 536, 65 537 and 131 070 times in a block: every sample of the first run lands in one cell,
    whose 16-bit counter ends at 0xFFFF exactly (i), or would have wrapped without the flush (ii-v); rejected samples
    advance the run but not the count (v)."""
    w, _, _ = case()
    z9 = W.split(w)["z"] + 9                                                  # the white noise
    four = np.tile(w["params_true"], (4, 1))
    four[1, z9] *= 1.01
    four[2, z9] *= 1.02
    four[3, z9] = np.nan
    seq = np.array(counter_sequences()[name])
    P = four[seq]
    ok = seq != 3
    n = int(ok.sum())
    assert len(seq) > RUN and (name == "v") == (n < len(seq))
    with open_case(accel_mod) as acc:
        _, st4, rows4 = gpu_rows(acc, four)
        assert list(st4) == [0, 0, 0, 1]
        assert np.all(rows4[0] < rows4[1]) and np.all(rows4[1] < rows4[2]), "a bin where min == max"
        truth = truth_of(rows4[seq[ok]], Q5)
        for nbits in (6, 4):
            with capi.Summary(acc, len(seq)) as s:
                _, st = s.push(P)
                assert np.array_equal(st == 0, ok)
                r = s.quantiles(P, Q5, nbits)
                tot = s.result()
            assert tot["n_used"] == n and tot["n_rejected"] == len(seq) - n
            assert np.array_equal(r["ranks"], ranks_of(Q5, n)) and r["bits_left"] == 0
            assert np.array_equal(bits(r["lo"]), bits(truth)) and np.array_equal(bits(r["hi"]), bits(truth)), (name, nbits)
