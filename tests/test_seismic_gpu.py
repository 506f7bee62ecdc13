"""The mode table's seismic indices on the GPU (tamcmc_modetable_indices_*, include/tamcmc_accel_seismic.h;
ModeTable.enable_indices / index_terms): Dnu, epsilon, nu_max, separations, second differences, d02 ... r10 as further
columns of the table.

Layouts: the global family (id 2) with lmax = 0 ... 3 and Nmax = 3, 4, 5 (three is the fewest radial modes, five the first
with a D10 and a D2NU at every degree), lmax = 3 with Nmax = 12 (more than 64 index columns: the lane loop's second trip),
lmax = 0 with Nmax = 70 (a fit longer than a wave), and the local family (id 11) with Nfl = (4, 3, 4, 2).  Frequencies follow
nu = Dnu (n + l / 2 + eps) - l (l + 1) D0; in a chain every frequency carries an AR(1) jitter of 0.05 (under 0.004 Dnu, far
inside the 0.35 assignment margin) and every height a relative one of 0.01.  Samples: 1, 2, 63, 64, 65 and B - 1, B, B + 1 for
the enabled table's own block size B = tm_mt_block(n_cols).

Checks.  (1) plan: columns(), the info and index_terms of every index column equal the numpy plan of
tests/seismic_reference.py, coefficient bits included.  (2) values bit for bit: derive()'s index columns equal the float64
restatement on derive()'s own base columns; D02 and DNU_NL equal the one subtraction of their two freq columns; the base
columns and the status equal those of an object without indices.  (3) every index column within 10 x its first-order
sensitivity to a relative 2^-50 change of each source of the long-double value.  (4) nothing else moves: result, quantiles,
ess, cov, corr, rank_diag of the base columns equal those of an object without indices; every result is independent of the
push split and of max_samples.  (5) downstream on the new columns: quantiles are order statistics of the derived column,
the ESS finish is ess_reference's on the library's lag products, cov of the ratio columns is within the modediag suite's
bound of the long-double sums.  (6) planted truths.  (7) status: +-inf accepted, NaN rejected.  (8) refusals.
test_zz_report prints the worst ratios."""
import math

import numpy as np
import pytest

import ess_reference as ER
import modediag_reference as DR
import modetable_reference as MR
import seismic_reference as SR
import workloads as W
from support import LD, bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
QS = np.array([0.0, 0.16, 0.5, 0.84, 1.0])
WORST = {"ld": 0.0, "truth": 0.0, "cov": 0.0, "corr": 0.0}
REPORT = []
BLOCK, BLOCK_BYTES = 4096, 1 << 26
DNU, EPS, D0, N0 = 60.0, 1.4, 0.9, 38          # workloads._layout_modes

GLOBAL = [(lmax, Nmax) for lmax in range(4) for Nmax in (3, 4, 5)] + [(3, 12), (0, 70)]
LAYOUTS = [("g%d-%d" % c) for c in GLOBAL] + ["local"]


local_layout = W.local_asymptotic


def layout(name):
    if name == "local":
        return local_layout()
    lmax, Nmax = (int(v) for v in name[1:].split("-"))
    return W.layout(2, lmax=lmax, Nmax=Nmax)


def heights_of(w):
    return range(int(w["plength"][0]))


def chain(w, n, seed, only=None, sigma=0.05):
    """n params rows around params_true: AR(1) jitter on every mode frequency (or on the params entries `only`), relative
    jitter on the heights."""
    cols = MR.layout(w["model_case"], w["plength"])
    P = np.tile(w["params_true"], (n, 1))
    fk = [int(k) for k in cols["param_index"][cols["param_index"] >= 0]] if only is None else list(only)
    for j, k in enumerate(fk):
        P[:, k] += ER.ar1(0.9 * j / max(len(fk) - 1, 1), n, sigma, seed * 1000 + j)
    if only is None:
        for j in heights_of(w):
            P[:, j] *= 1.0 + ER.ar1(0.5, n, 0.01, seed * 1000 + 500 + j)
    return P


def open_acc(accel_mod, w):
    return accel_mod.Accel(w["model_case"], w["plength"], w["x"], np.ones(w["x"].size))


def reference_plan(acc_mt_plain, w):
    cols = MR.layout(w["model_case"], w["plength"])
    ref, st = acc_mt_plain.derive(w["params_true"][None, :])
    assert st[0] == 0
    return cols, SR.plan(cols, ref[0])


def block_of(n_cols):
    fit = BLOCK_BYTES // (n_cols * 8)
    return BLOCK if fit >= BLOCK else max(fit, 1)


def check_values(tag, plan, nb, rows, rows_plain, st, st_plain):
    """Checks 2 and 3 on one derive() call."""
    terms, icols = plan["terms"], plan["cols"]
    assert rows.shape[1] == nb + len(terms) and rows_plain.shape[1] == nb, tag
    assert np.array_equal(bits(rows[:, :nb]), bits(rows_plain)) and np.array_equal(st, st_plain) and np.all(st == 0), tag
    want = SR.evaluate(terms, rows[:, :nb])
    got = rows[:, nb:]
    assert np.array_equal(bits(got), bits(want)), (tag, np.argwhere(bits(got) != bits(want))[:5])
    for j, (c, t) in enumerate(zip(icols, terms)):
        if c["kind"] in (SR.K["d02"], SR.K["dnu_nl"]):
            assert t["n_num"] == 2 and t["n_den"] == 0
            assert np.array_equal(bits(got[:, j]), bits(rows[:, t["src"][0]] - rows[:, t["src"][1]])), (tag, j)
    ld = SR.evaluate(terms, rows[:, :nb], LD)
    bound = (10 * LD(2.0) ** -50 * SR.sensitivity(terms, rows[:, :nb]))
    err = np.abs(got.astype(LD) - ld)
    assert np.all(bound > 0) and np.all(err <= bound), (tag, float(np.max(err / bound)))
    WORST["ld"] = max(WORST["ld"], float(np.max(err / bound)))


@pytest.mark.parametrize("name", LAYOUTS)
def test_plan_and_values(accel_mod, name):
    """Checks 1 to 3 of one layout, at every sample count."""
    w = layout(name)
    with open_acc(accel_mod, w) as acc, accel_mod.ModeTable(acc, 0) as plain, accel_mod.ModeTable(acc, 0) as mt:
        cols, plan = reference_plan(plain, w)
        nb = len(cols)
        assert mt.n_cols == nb == plain.n_cols
        info = mt.enable_indices(w["params_true"])
        ni = len(plan["terms"])
        assert mt.n_cols == nb + ni and ni >= 3 and plain.n_cols == nb
        for k in ("n_base_cols", "n_index_cols", "n_radial", "n_unassigned", "n_base"):
            assert info[k] == plan["info"][k], (name, k, info[k], plan["info"][k])
        assert bits(info["dnu_ref"]) == bits(plan["info"]["dnu_ref"]) and bits(info["eps_ref"]) == bits(plan["info"]["eps_ref"])
        assert 0.5 <= info["eps_ref"] < 1.5 and info["n_unassigned"] == 0 and mt.indices_info() == info
        if name != "local":
            assert info["n_base"] == N0 and abs(info["dnu_ref"] - DNU) < 1e-9 and abs(info["eps_ref"] - EPS) < 1e-9
            lmax, Nmax = GLOBAL[LAYOUTS.index(name)]
            if (lmax, Nmax) == (3, 12):
                assert ni > 64
            if Nmax == 70:
                assert plan["terms"][0]["n_num"] == 70 and plan["terms"][1]["n_num"] + plan["terms"][1]["n_den"] == 140
            if Nmax >= 5:
                kinds = set(int(k) for k in plan["cols"]["kind"])
                assert SR.K["d2nu"] in kinds and (lmax < 1 or SR.K["d10"] in kinds)
        got_cols = mt.columns()
        assert np.array_equal(got_cols[:nb], cols) and np.array_equal(got_cols[nb:], plan["cols"]), name
        assert np.array_equal(plain.columns(), cols)
        for j, t in enumerate(plan["terms"]):
            g = mt.index_terms(nb + j)
            assert (g["n_num"], g["n_den"]) == (t["n_num"], t["n_den"]) and bits(g["offset"]) == bits(t["offset"]), (name, j)
            assert np.array_equal(g["src"], t["src"]) and np.array_equal(g["wsrc"], t["wsrc"]) and np.array_equal(bits(g["coef"]), bits(t["coef"])), (name, j)
        B = block_of(nb + ni)
        P = chain(w, B + 1, seed=LAYOUTS.index(name) + 1)
        for n in (1, 2, 63, 64, 65, B - 1, B, B + 1):
            rows, st = mt.derive(P[:n])
            rows_plain, st_plain = plain.derive(P[:n])
            check_values((name, n), plan, nb, rows, rows_plain, st, st_plain)
        assert mt.seismic_kernel_time() == (0.0, 0) and plain.seismic_kernel_time() == (0.0, 0)       # derive() is not timed
        mt.push(P[:65])
        ms, launches = mt.seismic_kernel_time()
        assert ms > 0.0 and launches == 1 and mt.kernel_time()[1] == 2
        mt.reset()
        assert mt.seismic_kernel_time() == (0.0, 0) and mt.n_cols == nb + ni and mt.indices_info() == info      # reset keeps the plan


def collect(mt, sel, L=0):
    """Everything a table returns, of all its columns; cov, corr and rank_diag of the columns sel."""
    r = {("result", k): v for k, v in mt.result().items()}
    q = mt.quantiles(QS)
    r.update({("q", "ranks"): q["ranks"], ("q", "values"): q["values"]})
    e = mt.ess(L)
    r.update({("ess", k): v for k, v in e.items()})
    r[("acov",)] = mt.acov()
    r[("cov",)] = mt.cov(sel)
    r[("corr",)] = mt.corr(sel)
    rk = mt.rank_diag(L, sel)
    r.update({("rank", k): v for k, v in rk.items()})
    return r


def same(a, b, tag, cols=None, skip=()):
    """Bit equality of two collect() results; with cols, a's per-column arrays are cut to those columns first."""
    assert a.keys() == b.keys(), tag
    for k in a:
        if k in skip or k[-1] in skip:
            continue
        x, y = a[k], b[k]
        if cols is not None and isinstance(x, np.ndarray) and k[0] in ("result", "q", "ess", "acov") and x.ndim >= 1 and x.shape[-1] != y.shape[-1]:
            x = x[..., cols]
        if isinstance(x, np.ndarray) and x.dtype == np.float64:
            assert np.array_equal(bits(x), bits(y)), (tag, k)
        elif isinstance(x, float):
            assert bits(x) == bits(y), (tag, k)
        else:
            assert np.array_equal(x, y), (tag, k)


TOTALS = ("n_cols", "min_ess", "col_min_ess", "max_rhat", "col_max_rhat", "n_truncated", "n_constant", "n_rhat_high",
          "min_ess_bulk", "col_min_ess_bulk", "min_ess_tail", "col_min_ess_tail")


@pytest.mark.parametrize("name,n", [("g0-3", 65), ("g1-4", 64), ("g2-5", 65), ("g3-5", 63), ("g3-12", 65), ("g0-70", 65), ("local", 65), ("g2-5", None)])
def test_nothing_else_moves_and_downstream(accel_mod, name, n):
    """Checks 4 and 5.  n = None: B + 1 samples, pushes that straddle the block."""
    w = layout(name)
    with open_acc(accel_mod, w) as acc:
        with accel_mod.ModeTable(acc, 0) as probe:
            cols, plan = reference_plan(probe, w)
        nb, ni = len(cols), len(plan["terms"])
        B = block_of(nb + ni)
        big = n is None
        n = B + 1 if big else n
        P = chain(w, n, seed=77 + LAYOUTS.index(name))
        sel = np.concatenate([DR.headline(cols)[:40], np.arange(nb, nb + ni)]).astype(np.int32) if nb + ni > 200 else np.arange(nb + ni, dtype=np.int32)
        sel_base = sel[sel < nb]
        splits = [[n], [B - 1, 2], [1, B - 1, 1]] if big else [[n], [1] * n, [n // 2, n - n // 2]]
        results = []
        for k, split in enumerate(splits):
            with accel_mod.ModeTable(acc, n + (37 if k == 1 else 0)) as mt:
                mt.enable_indices(w["params_true"])
                at = 0
                for m in split:
                    assert np.all(mt.push(P[at:at + m]) == 0)
                    at += m
                results.append(collect(mt, sel))
                if k == 0:
                    rows, _ = mt.derive(P)
        with accel_mod.ModeTable(acc, n) as plain:
            plain.push(P)
            base = collect(plain, sel_base)
        for k in range(1, len(results)):
            same(results[0], results[k], (name, n, "split", k))
        r = results[0]
        assert r[("result", "n_used")] == n and r[("result", "n_cols")] == nb + ni
        # (4) the base columns against the object without indices: per-column arrays cut to the base columns; the totals
        # are over all columns and may move
        cut = {k: v for k, v in r.items()}
        keep = np.flatnonzero(sel < nb)
        cut[("cov",)], cut[("corr",)] = r[("cov",)][np.ix_(keep, keep)], r[("corr",)][np.ix_(keep, keep)]
        for k in list(cut):
            if k[0] == "rank" and isinstance(cut[k], np.ndarray):
                cut[k] = cut[k][..., keep]
        same(cut, base, (name, n, "base"), cols=np.arange(nb), skip=TOTALS)
        # (5) downstream on the new columns
        idx = np.arange(nb, nb + ni)
        srt = np.sort(rows[:, idx], axis=0)
        ranks = r[("q", "ranks")]
        assert np.array_equal(bits(r[("q", "values")][:, idx]), bits(srt[ranks, :])), (name, n)
        A = r[("acov",)]
        tau, ess, cutl = ER.finish(A[:, idx], n)
        floor = 1.0 / math.log10(float(n))
        assert np.array_equal(cutl, r[("ess", "cut")][idx])
        for got, want in ((r[("ess", "tau")][idx], tau), (r[("ess", "ess")][idx], ess)):
            on_floor = np.abs(tau - floor) <= 4 * U * floor
            ok = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want)) | (on_floor & (np.abs(got - want) <= 4 * U * np.abs(want)))
            assert np.all(ok), (name, n, np.flatnonzero(~ok))
        ratio = np.flatnonzero(np.isin(mt_kinds(cols, plan), [SR.K[k] for k in SR.RATIOS])).astype(np.int32)
        if ratio.size:
            with accel_mod.ModeTable(acc, n) as mt:
                mt.enable_indices(w["params_true"])
                mt.push(P)
                cov, mean = mt.cov(ratio), mt.result()["mean"]
            assert np.array_equal(bits(cov), bits(cov.T))
            d, e = DR.centred(rows[:, ratio], mean[ratio])
            Sq, sb = DR.cov_sums(d, e)
            sb = sb + U * np.abs(Sq).astype(np.float64)
            serr = np.abs(cov.astype(LD) * LD(n - 1) - Sq).astype(np.float64)
            assert np.all(serr <= 10 * sb), (name, n, float(np.max(serr[sb > 0] / sb[sb > 0])))
            WORST["cov"] = max(WORST["cov"], float(np.max(serr[sb > 0] / sb[sb > 0])))
            # neighbouring ratios share frequencies: the matrix is far from diagonal
            if ratio.size >= 2 and not big:
                c = r[("corr",)]
                pos = {int(col): i for i, col in enumerate(sel)}
                off = [abs(c[pos[int(a)], pos[int(b)]]) for a, b in zip(ratio[:-1], ratio[1:]) if int(a) in pos and int(b) in pos]
                REPORT.append(f"{name} n={n}: largest |corr| of neighbouring ratio columns {max(off):.3f}")


def mt_kinds(cols, plan):
    return np.concatenate([cols["kind"], plan["cols"]["kind"]])


def find(cols, plan, kind, order=None, l=None):
    k = mt_kinds(cols, plan)
    o = np.concatenate([cols["order"], plan["cols"]["order"]])
    ll = np.concatenate([cols["l"], plan["cols"]["l"]])
    code = SR.K[kind] if kind in SR.K else MR.K[kind]
    m = (k == code) & (True if order is None else o == order) & (True if l is None else ll == l)
    return np.flatnonzero(m)


def test_planted_exact_pattern(accel_mod):
    """Check 6a: no jitter; DNU_FIT, EPSILON, D02 = 6 D0 and R02 = 6 D0 / Dnu within the bound of check 3 of the exact values
    (the frequencies in the params row are the pattern rounded to double: a relative change far below 2^-50)."""
    w = layout("g3-5")
    with open_acc(accel_mod, w) as acc, accel_mod.ModeTable(acc, 0) as plain, accel_mod.ModeTable(acc, 0) as mt:
        cols, plan = reference_plan(plain, w)
        nb = len(cols)
        mt.enable_indices(w["params_true"])
        rows, st = mt.derive(np.tile(w["params_true"], (3, 1)))
    assert np.all(st == 0) and np.array_equal(bits(rows[0]), bits(rows[2]))
    bound = (10 * LD(2.0) ** -50 * SR.sensitivity(plan["terms"], rows[:1, :nb]))[0]
    truth = {"dnu_fit": DNU, "epsilon": EPS, "d02": 6 * D0, "r02": 6 * D0 / DNU, "dnu_nl": DNU, "d13": 10 * D0, "d01": 2 * D0, "d10": 2 * D0,
             "r13": 10 * D0 / DNU, "r01": 2 * D0 / DNU, "r10": 2 * D0 / DNU, "d2nu": 0.0}
    seen = set()
    for j, c in enumerate(plan["cols"]):
        kind = SR.ALL_KINDS[c["kind"]]
        if kind in truth:
            err = abs(LD(rows[0, nb + j]) - LD(truth[kind]))
            assert err <= bound[j], (kind, j, float(err / bound[j]))
            WORST["truth"] = max(WORST["truth"], float(err / bound[j]))
            seen.add(kind)
    assert {"dnu_fit", "epsilon", "d02", "r02"} <= seen


def test_planted_shared_frequency_and_ar1(accel_mod):
    """Check 6b, 6c.  Only nu_{n,1} moves: R02(n) = d02 / (nu_{n,1} - nu_{n-1,1}) and R02(n+1) = d02' / (nu_{n+1,1} - nu_{n,1})
    move in opposite directions, to first order corr = -1; the library's value is within the modediag suite's bound of the
    long-double one.  A radial frequency with an AR(1) phi = 0.8 jitter gives D02 of its order the ESS of that sequence."""
    n, phi = 4000, 0.8
    w = layout("g2-5")
    with open_acc(accel_mod, w) as acc:
        with accel_mod.ModeTable(acc, 0) as plain:
            cols, plan = reference_plan(plain, w)
        nb = len(cols)
        order = N0 + 2                                       # the middle of the ladder
        k1 = int(cols["param_index"][find(cols, plan, "freq", order - N0, 1)[0]])
        ra, rb = int(find(cols, plan, "r02", order)[0]), int(find(cols, plan, "r02", order + 1)[0])
        P = chain(w, n, seed=5, only=[k1], sigma=0.05)
        with accel_mod.ModeTable(acc, n) as mt:
            mt.enable_indices(w["params_true"])
            mt.push(P)
            rows, _ = mt.derive(P)
            corr, cov, mean = mt.corr([ra, rb]), mt.cov([ra, rb]), mt.result()["mean"]
        d, e = DR.centred(rows[:, [ra, rb]], mean[[ra, rb]])
        Sq, sb = DR.cov_sums(d, e)
        sb = sb + U * np.abs(Sq).astype(np.float64)
        rq, rbnd = DR.corr(Sq, 10 * sb)
        cerr = abs(float(LD(corr[0, 1]) - rq[0, 1]))
        assert cerr <= rbnd[0, 1] + 8 * U and corr[0, 1] != 0.0 and bits(corr[0, 1]) == bits(corr[1, 0])
        WORST["corr"] = max(WORST["corr"], cerr / (rbnd[0, 1] + 8 * U))
        REPORT.append(f"corr(R02(n), R02(n+1)) with only nu_(n,1) moving: {corr[0, 1]:.6f}; long double {float(rq[0, 1]):.6f}; first order -1")
        assert abs(corr[0, 1] + 1.0) < 0.01
        # the AR(1) radial frequency
        k0 = int(cols["param_index"][find(cols, plan, "freq", order - N0, 0)[0]])
        c02 = int(find(cols, plan, "d02", order)[0])
        P = np.tile(w["params_true"], (n, 1))
        P[:, k0] += ER.ar1(phi, n, 0.01, seed=1)
        with accel_mod.ModeTable(acc, n) as mt:
            mt.enable_indices(w["params_true"])
            mt.push(P)
            r, res, A = mt.ess(255), mt.result(), mt.acov()
            rows, _ = mt.derive(P)
        dd, ee = DR.centred(rows[:, [c02]], res["mean"][c02])
        Aq, bound = DR.lag(dd, ee, 255)
        assert np.all(np.abs(A[:, c02].astype(LD) - Aq[:, 0]).astype(np.float64) <= 10 * bound[:, 0])
        expect = n * (1 - phi) / (1 + phi)
        REPORT.append(f"AR(1) phi 0.8 on a radial frequency: ess of its D02 {r['ess'][c02]:.1f}, expected {expect:.1f}; the sequence itself "
                      f"{ER.ess_of_sequence(P[:, k0], 255)[1]:.1f}")
        assert abs(r["ess"][c02] - expect) <= 0.15 * expect


def test_status(accel_mod):
    """Check 7: two equal radial frequencies give R10 = +-inf and the sample stays accepted; numerator and denominator
    vanishing together give a NaN: TAMCMC_CHAIN_NAN, rejected, counted; the chain with such rows returns the bits of the
    chain without them."""
    w = layout("g3-5")
    with open_acc(accel_mod, w) as acc:
        with accel_mod.ModeTable(acc, 0) as plain:
            cols, plan = reference_plan(plain, w)
        nb = len(cols)
        fk = lambda l, k: int(cols["param_index"][find(cols, plan, "freq", k, l)[0]])
        order = N0 + 2
        r10, r13 = int(find(cols, plan, "r10", order)[0]), int(find(cols, plan, "r13", order)[0])
        P = chain(w, 12, seed=9)
        inf_row = P[3].copy()
        inf_row[fk(0, 3)] = inf_row[fk(0, 2)]                 # nu_{n+1,0} = nu_{n,0}: the denominator of R10(n), R13(n)
        nan_row = inf_row.copy()
        nan_row[fk(1, 2)] = nan_row[fk(3, 1)]                 # nu_{n,1} = nu_{n-1,3}: the numerator of R13(n) too
        with accel_mod.ModeTable(acc, 0) as mt:
            mt.enable_indices(w["params_true"])
            rows, st = mt.derive(np.stack([inf_row, nan_row]))
            assert list(st) == [0, 1] and np.isinf(rows[0, r10]) and np.isinf(rows[0, r13]) and not np.any(np.isnan(rows[0]))
            assert np.isnan(rows[1, r13]) and np.isinf(rows[1, r10]) and not np.any(np.isnan(rows[1, :nb]))
            st = mt.push(inf_row[None, :])
            t = mt.result()
            assert st[0] == 0 and t["n_used"] == 1 and t["n_rejected"] == 0 and np.isinf(t["max"][r10])
        Pin = np.concatenate([P[:4], nan_row[None, :], P[4:9], nan_row[None, :], P[9:]])
        sel = np.arange(nb, nb + len(plan["terms"]), dtype=np.int32)
        with accel_mod.ModeTable(acc, 12) as mt, accel_mod.ModeTable(acc, 12) as clean:
            mt.enable_indices(w["params_true"])
            clean.enable_indices(w["params_true"])
            st = mt.push(Pin)
            assert list(np.flatnonzero(st)) == [4, 10] and np.all(st[[4, 10]] == 1)
            clean.push(P)
            got, want = collect(mt, sel), collect(clean, sel)
            assert got[("result", "n_used")] == 12 and got[("result", "n_rejected")] == 2 and want[("result", "n_rejected")] == 0
            same(got, want, "status", skip=("n_rejected",))


def test_refusals(accel_mod):
    """Check 8."""
    E = accel_mod.capi.E_INVALID
    w = layout("g1-3")
    ref = w["params_true"]

    def refused(fn):
        with pytest.raises(accel_mod.AccelError) as e:
            fn()
        assert e.value.code == E

    with open_acc(accel_mod, w) as acc:
        P = chain(w, 6, seed=3)
        with accel_mod.ModeTable(acc, 8) as mt:
            nb = mt.n_cols
            refused(lambda: mt.indices_info())
            refused(lambda: mt.index_terms(0))
            info = mt.enable_indices(ref)
            refused(lambda: mt.enable_indices(ref))                                   # a second call
            assert mt.indices_info() == info and mt.n_cols == nb + info["n_index_cols"]
            refused(lambda: mt.index_terms(0))
            refused(lambda: mt.index_terms(nb - 1))                                   # a base column
            refused(lambda: mt.index_terms(mt.n_cols))
            ce = int(np.flatnonzero(mt.columns()["kind"] == SR.K["epsilon"])[0])
            t = mt.index_terms(ce)                                                    # epsilon: 3 + 3 terms
            nn, nd = accel_mod.capi.C.c_int32(-1), accel_mod.capi.C.c_int32(-1)
            buf_i, buf_d = np.full(8, 7, dtype=np.int32), np.full(8, 7.0)
            ip, dp = accel_mod.capi._iptr, accel_mod.capi._dptr
            rc = acc._lib.tamcmc_modetable_index_terms(mt._mt, ce, 5, accel_mod.capi.C.byref(nn), accel_mod.capi.C.byref(nd), ip(buf_i), ip(buf_i),
                                                       dp(buf_d), dp(buf_d))
            assert rc == E and (nn.value, nd.value) == (t["n_num"], t["n_den"]) == (3, 3) and np.all(buf_i == 7) and np.all(buf_d == 7.0)   # a short cap
            assert acc._lib.tamcmc_modetable_indices_enable(mt._mt, acc.Nparams + 1, dp(ref), accel_mod.capi.C.byref(accel_mod.capi.SeismicInfo())) == E
        with accel_mod.ModeTable(acc, 8) as mt:
            mt.push(P[:2])
            refused(lambda: mt.enable_indices(ref))                                   # after a push
            mt.reset()
            assert mt.enable_indices(ref)["n_index_cols"] > 0                           # ... and after the reset that follows
        with accel_mod.ModeTable(acc, 8) as mt:
            mt.push(P[:5])
            mt.ess(0)
            mt.reset()
            refused(lambda: mt.enable_indices(ref))                                   # after an ess call: its buffers exist
            assert mt.n_cols == nb and mt.derive(P[:1])[0].shape == (1, nb)
        with accel_mod.ModeTable(acc, 0) as mt:
            bad = ref.copy()
            bad[-2] = -1.0                                                            # negative trunc_c: an empty window
            assert mt.derive(bad[None, :])[1][0] == 2
            refused(lambda: mt.enable_indices(bad))
            assert mt.n_cols == nb and mt.enable_indices(ref)["n_radial"] == 3       # the refusal left the object as it was
    w5 = layout("g1-5")
    with open_acc(accel_mod, w5) as acc, accel_mod.ModeTable(acc, 0) as mt:
        cols = MR.layout(w5["model_case"], w5["plength"])
        f0 = [int(k) for k in cols["param_index"][(cols["kind"] == MR.K["freq"]) & (cols["l"] == 0)]]
        gap = w5["params_true"].copy()
        gap[f0[3:]] += DNU                                                            # a missing radial order
        assert mt.derive(gap[None, :])[1][0] == 0
        refused(lambda: mt.enable_indices(gap))
        assert mt.enable_indices(w5["params_true"])["n_radial"] == 5
    w2 = W.layout(2, lmax=1, Nmax=2)
    with open_acc(accel_mod, w2) as acc, accel_mod.ModeTable(acc, 0) as mt:
        refused(lambda: mt.enable_indices(w2["params_true"]))                         # two radial modes


def test_zz_report():
    """The worst ratios of this module's cases, and the planted truths' lines."""
    print("seismic worst error / bound: values against long double %.3g, planted truths %.3g (of 1); cov of the ratios %.3g (of the 10 allowed); "
          "planted corr %.3g (of 1)" % (WORST["ld"], WORST["truth"], WORST["cov"], WORST["corr"]))
    for line in REPORT:
        print(line)
    assert WORST["ld"] > 0.0
