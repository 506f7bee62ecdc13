"""The posterior mode table on the GPU (tamcmc_modetable_*, include/tamcmc_accel.h; tamcmc_amd.ModeTable).

A table row is a complete description of the sample's mode spectrum, so it is checked against the oracle without a second
derivation: the model row rebuilt from the table row plus the noise parameters (tests/modetable_reference.py) stays, in every
bin, within RTOL_MODEL |M_i| + 10 S_i of the oracle's row and of the library's own model_explicit row, S_i being the bin's
first-order sensitivity to a relative 2^-50 change of every table entry.  Then the identities the columns obey among
themselves, the status codes, the statistics against the library's own derived rows in long double, the quantiles against a
sort, and the independence of every result bit from how the samples are pushed."""
import numpy as np
import pytest

import layouts
import modetable_reference as MR
import workloads as W
from modetable_support import QS, check_case, check_quantiles, check_statistics, collect, open_acc, same_results
from support import bits

pytestmark = pytest.mark.gpu

WORST = {}
CASES = {}
for (_name, _mid, _lmax, _v, _g) in layouts.matrix_cases():
    if _g == "fused" or (_mid in (2, 9, 13, 11) and _lmax == 3):
        CASES.setdefault(_mid, []).append((_name, _lmax, _v, _g))


@pytest.mark.parametrize("mid", sorted(CASES))
def test_reconstruction_and_identities(accel_mod, mid):
    """Items 1 and 2: every case of the layout matrix on the fused grid, the three variants of ids 2, 9, 13 and 11 on the
    tiled grid, three perturbed rows each.  amplitude: the bound is 1 ulp of numpy's sqrt((pi height) width); the largest
    distance is printed, and on the MI355X it is 0 in every case (the device's sqrt is correctly rounded and the product is
    formed in the same order, without contraction)."""
    worst, amp = 0.0, 0
    for name, lmax, v, g in CASES[mid]:
        w = layouts.matrix_case(mid, lmax, v, g)
        r, a = check_case(accel_mod, w, W.perturbed(w, layouts.NCHAINS))
        worst, amp = max(worst, r), max(amp, a)
    WORST[mid] = worst
    print(f"modetable id {mid}: {len(CASES[mid])} cases, worst |R - M| / bound = {worst:.3g}, amplitude within {amp} ulp")
    assert amp <= 1


@pytest.mark.parametrize("lmax,Nmax,n_mult", [(2, 21, 63), (3, 16, 64), (0, 65, 65), (3, 64, 256), (0, 2, 2)])
def test_multiplet_counts_around_the_wave_loop(accel_mod, lmax, Nmax, n_mult):
    """Item 3: 63, 64 and 65 multiplets (one wave derives 64 at a time), TM_MAXMULT = 256, and 2."""
    w = W.layout(2, lmax=lmax, Nmax=Nmax)
    assert len(MR.multiplets(2, w["plength"])) == n_mult
    worst, amp = check_case(accel_mod, w, W.perturbed(w, 2))
    print(f"modetable {n_mult} multiplets: worst ratio {worst:.3g}, amplitude within {amp} ulp")
    assert amp <= 1


def small_case():
    """id 2, lmax 1, Nmax 2: 48 columns"""
    w = W.layout(2, lmax=1, Nmax=2)
    assert len(MR.layout(2, w["plength"])) == 48
    return w


def test_status_and_skip(accel_mod):
    """Item 4: rows with a NaN frequency, a NaN width, the inclination pair both 0 and an empty window among healthy rows get
    the status eval_batch gives them and are counted as rejected; the statistics are those of the chain without them, bit
    for bit; the same for rows named by skip."""
    w = W.make(2, Nx=3000)
    b = W.split(w)
    P = W.perturbed(w, 9, scale=0.002)
    P[1, b["q"] + 1] = -1.0                                   # negative trunc_c -> empty window
    P[3, b["Nmax"] + b["lmax"] + 2] = np.nan                  # a frequency
    P[4, b["w"] + 1] = np.nan                                 # a width
    P[6, b["s"] + 3] = P[6, b["s"] + 4] = 0.0                 # atan(0 / 0)
    bad = [1, 3, 4, 6]
    good = [k for k in range(9) if k not in bad]
    with open_acc(accel_mod, w) as acc:
        _, st_eval = acc.eval_batch(P, np.ones(9))
        with accel_mod.ModeTable(acc, 16) as mt, accel_mod.ModeTable(acc, 16) as ref:
            rows, st_d = mt.derive(P)
            st = mt.push(P)
            ref.push(P[good])
            got, want = collect(mt), collect(ref)
            assert np.array_equal(st, st_eval) and np.array_equal(st_d, st_eval), (st, st_d, st_eval)
            assert st[1] == 2 and st[6] == 1 and np.all(st[bad] != 0) and np.all(st[good] == 0)
            assert np.all(np.isnan(rows[6]).any()) and got["n_used"] == 5 and got["n_rejected"] == 4 and want["n_rejected"] == 0
            got.pop("n_rejected"); want.pop("n_rejected")
            same_results(got, want)
            # skip: two healthy rows out, one bad row named as well
            skip = np.zeros(9, dtype=np.int32)
            skip[[0, 7, 3]] = 1
            mt.reset(); ref.reset()
            st2 = mt.push(P, skip=skip)
            ref.push(P[[2, 5, 8]])
            got, want = collect(mt), collect(ref)
            assert np.array_equal(st2, st_eval) and got["n_used"] == 3 and got["n_rejected"] == 6
            got.pop("n_rejected"); want.pop("n_rejected")
            same_results(got, want)


# 1, 2, 3, 37, 1000, 70 001: item 5.  255, 256, 257: the quantile kernel's 256 threads stride over a column, so a sweep
# ends exactly at, one before and one past a whole number of strides.  4095, 4096, 4097: the block of a push (the fold
# appends to the table block by block).  The kernel has no counter flush (32-bit LDS counters, fewer than 2^31 samples), and
# its pass count, ceil(bit_length(key(max) - key(min)) / 8), depends on a column's spread, not on n: the 48 columns hold
# constant columns (0 passes), integer-valued window edges, heights and frequencies (6 to 8 passes).
@pytest.mark.parametrize("n", [1, 2, 3, 37, 255, 256, 257, 1000, 4095, 4096, 4097, 70001])
def test_statistics_and_quantiles(accel_mod, n):
    w = small_case()
    P = W.perturbed(w, n, scale=0.01, seed=n)
    with open_acc(accel_mod, w) as acc, accel_mod.ModeTable(acc, n) as mt:
        rows, st = mt.derive(P)
        assert np.array_equal(mt.push(P), st)
        res = collect(mt)
    keep = st == 0
    assert keep.sum() >= n - n // 100 and res["n_rejected"] == n - keep.sum()
    check_statistics(n, res, rows[keep])
    check_quantiles(n, res, rows[keep])


def test_repeated_rows(accel_mod):
    """All rows equal (one row fifty times): sd exactly 0, every quantile the value.  Every row twice: statistics and quantiles
    of the doubled chain."""
    w = small_case()
    P = W.perturbed(w, 37, scale=0.01, seed=5)
    with open_acc(accel_mod, w) as acc, accel_mod.ModeTable(acc, 100) as mt:
        one, st = mt.derive(P[:1])
        assert st[0] == 0
        mt.push(np.repeat(P[:1], 50, axis=0))
        res = collect(mt)
        assert res["n_used"] == 50 and np.all(res["sd"] == 0.0)
        for k in ("mean", "min", "max"):
            assert np.array_equal(bits(res[k]), bits(one[0])), k
        assert np.array_equal(bits(res["q_values"]), bits(np.tile(one[0], (QS.size, 1))))
        mt.reset()
        P2 = np.repeat(P, 2, axis=0)
        rows, st = mt.derive(P2)
        mt.push(P2)
        res = collect(mt)
        assert np.all(st == 0)
        check_statistics("twice", res, rows)
        check_quantiles("twice", res, rows)


def test_refusals(accel_mod):
    """Quantiles before any push and with max_samples = 0 are refused; a push past max_samples is refused whole and changes
    nothing; ids 0 and 1 have no table; the context cannot be destroyed under a live table."""
    E = accel_mod.capi.E_INVALID
    w = small_case()
    P = W.perturbed(w, 12, scale=0.01, seed=9)
    with open_acc(accel_mod, w) as acc:
        with accel_mod.ModeTable(acc, 10) as mt:
            with pytest.raises(accel_mod.AccelError) as e:
                mt.quantiles(QS)
            assert e.value.code == E
            mt.push(P[:7])
            before = collect(mt)
            with pytest.raises(accel_mod.AccelError) as e:
                mt.push(P[7:])                                 # 7 + 5 > 10
            assert e.value.code == E
            same_results(collect(mt), before)
            mt.push(P[7:10])                                   # exactly full
            assert mt.result()["n_used"] == 10
            for bad_q in ([], [1.5], [np.nan], list(np.linspace(0, 1, 9))):
                with pytest.raises(accel_mod.AccelError):
                    mt.quantiles(bad_q)
            with pytest.raises(ValueError):
                mt.push(P[:, :-1])
            assert acc._lib.tamcmc_ctx_destroy(acc._ctx) == E  # refused under a live table
            assert mt.result()["n_used"] == 10
        with accel_mod.ModeTable(acc, 0) as mt:
            mt.push(P)
            res = mt.result()
            assert res["n_used"] == 12 and res["n_mult"] == 4
            with pytest.raises(accel_mod.AccelError) as e:
                mt.quantiles(QS)
            assert e.value.code == E
        with pytest.raises(accel_mod.AccelError):
            accel_mod.ModeTable(acc, -1)
    for mid in (0, 1):
        g = W.any_model(mid, Nx=512)
        with open_acc(accel_mod, g) as acc:
            with pytest.raises(accel_mod.AccelError) as e:
                accel_mod.ModeTable(acc)
            assert e.value.code == E


def test_bit_for_bit_independence_of_the_pushes(accel_mod):
    """Item 7: rows, status, statistics and quantiles are the same bits for one push, pushes of 1, of 7 and of 4097, and after a
    reset followed by the same pushes; a Summary, an eval_batch with gradient and a model_explicit on the same context return
    the same bits before, beside and after the table."""
    w = small_case()
    n = 4200
    P = W.perturbed(w, n, scale=0.01, seed=21)
    b = W.split(w)
    P[[5, 4096, 4199], b["q"] + 1] = -1.0                      # rejected rows, one either side of the block edge
    skip = np.zeros(n, dtype=np.int32)
    skip[[0, 4095, 4097]] = 1
    with open_acc(accel_mod, w) as acc0:
        m_true, _ = acc0.model_explicit(w["params_true"])
    y = m_true * (1.0 + 0.3 * np.sin(np.arange(m_true.size)))

    def neighbours(acc):
        acc.set_vars(w["index_to_relax"])
        with accel_mod.Summary(acc) as sm:
            sm.push(P[:40])
            r = sm.result()
        logL, st, g = acc.eval_batch(P[:8], np.linspace(1.0, 3.0, 8), grad=True)
        m, _ = acc.model_explicit(P[2])
        r.update(logL=logL, st=st, grad=g, model=m)
        return r

    with open_acc(accel_mod, w, y) as acc:
        base = neighbours(acc)
        with accel_mod.ModeTable(acc, n) as mt:
            rows, st = mt.derive(P)
            same_results(neighbours(acc), base)
            results = []
            for size in (n, 4097, 7, 1):
                for again in (False, True):
                    if again and size == 1:
                        continue
                    st_p = np.concatenate([mt.push(P[k:k + size], skip=skip[k:k + size]) for k in range(0, n, size)])
                    assert np.array_equal(st_p, st), size
                    results.append(collect(mt))
                    mt.reset()
                    assert mt.result()["n_used"] == 0
                r2 = np.concatenate([mt.derive(P[k:k + size])[0] for k in range(0, n, size)]) if size != 1 else rows
                assert np.array_equal(bits(r2), bits(rows)), size
            for r in results[1:]:
                same_results(r, results[0])
            keep = (st == 0) & (skip == 0)
            assert results[0]["n_used"] == keep.sum() == n - 6 and results[0]["n_rejected"] == 6
            check_statistics("pushes", results[0], rows[keep])
            check_quantiles("pushes", results[0], rows[keep])
            same_results(neighbours(acc), base)
            ms, launches = mt.kernel_time()
            assert ms == 0.0 and launches == 0                  # reset put it back
            mt.push(P[:10])
            ms, launches = mt.kernel_time()
            assert ms > 0.0 and launches == 2
        same_results(neighbours(acc), base)


def test_zz_report_worst_ratio():
    """Not a check: the line README quotes (run after the reconstruction cases of this module)."""
    if WORST:
        print("modetable worst |R - M| / bound per id: " + ", ".join(f"{k}: {v:.3g}" for k, v in sorted(WORST.items())) +
              f"; overall {max(WORST.values()):.3g}")
