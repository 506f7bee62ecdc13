"""The mode table's derive kernel, its status rule and the seismic indices at the parameter values where the derivation
changes branch or degenerates (tests/specialcases.py: the rows of the eval suite's special-values test), and on the
reference's own input files.

Ids 2, 3, 6, 7, 8, 9, 10, 11, 12, 13, 14, each with asym = 0, asym = 25 and do_amp, on 3000 bins (the grid only enters
through the truncation window); one derive / push per (id, variant) over all its cases.  Per case row:

  1  status: derive's and push's status equal eval_batch's of the same rows at T = 1 -- every row, the id 9 width overflow
     included (its widths reach exp(364): finite columns, an infinite square, TAMCMC_CHAIN_NAN by the table's own rule) --
     and the oracle's wherever the eval suite asserts that (everywhere but that overflow).  The header names
     one exception, "finite columns, overflowing sum"; test_the_named_exception asserts it case by case.
  2  reconstruction: every row with status 0 whose oracle row is finite rebuilds the oracle's and model_explicit's model row
     within modetable_reference.bound.  At most 2 cases per (id, variant) are left out, each because the oracle's status is
     not 0 or its row is not finite; their names are pinned per (id, variant) and the totals asserted: of 972 rows 943 are
     rebuilt, 28 left out, and 1 (id 9, asym = 0, 'W[1]=W[0]') has a finite oracle row but is rejected by the table as by
     eval_batch, so there is nothing to rebuild.  An oracle row with a NaN means a status != 0 here.
  3  identities: check_identities on every status-0 row; the inclination column against a long-double restatement of the
     header's rule within 4 ulp; splitting exactly +0 for l = 0 and never negative; height, h_m and width never negative,
     never -0.
  4  rejected rows leave no trace: the whole case list pushed equals, bit for bit, its status-0 rows pushed alone -- result,
     quantiles, ess, cov, rank_diag, hist, hpd; n_rejected counts the rest.
  5  seismic indices (ids 2 and 11): the index columns of the special rows equal seismic_reference.evaluate on the row's own
     base columns bit for bit; a NaN index gives TAMCMC_CHAIN_NAN, an infinite one stays accepted.
  6  the reference's .model files (both readers, every slice of the local file): checks 1 to 3 on chains_around(s, 4).
test_zz_report prints the worst ratios and the counts."""
import numpy as np
import pytest

import modetable_reference as MR
import seismic_reference as SR
import workloads as W
from modetable_support import QS, ULP, check_identities, open_acc, same_results
from specialcases import VARIANTS, cases
from support import CFG, DATA, LD, MODEL, REF_MODEL_FILES, bits, chains_around, load_on_flat_spectrum, pyorc
from tamcmc_amd.setup_io import Setup, model_file_slices

pytestmark = pytest.mark.gpu

IDS = [2, 3, 6, 7, 8, 9, 10, 11, 12, 13, 14]
ATAN_IDS, GIVEN_IDS = (2, 9, 10, 11), (3, 6, 7, 8)
PI_LD = LD("3.141592653589793238462643383279502884")
K = MR.K
RUNS = {}
REPORT = {"ratio": {}, "inc_ulp": 0.0, "rows": 0, "rebuilt": 0, "left_out": 0, "not_rebuilt": 0, "exceptions": [], "rejected": 0, "inf_index": 0,
          "nan_index": 0}


def collect_all(mt):
    """Everything check 4 compares: one dict of dicts."""
    out = {"result": mt.result()}
    n = out["result"]["n_used"]
    if n >= 1:
        out["quantiles"] = mt.quantiles(QS)
        out["hist"] = mt.hist(16)
    if n >= 4:
        out["hpd"] = mt.hpd([0.5, 0.95])
        out["ess"] = mt.ess()
        out["cov"] = {"cov": mt.cov()}
        out["rank_diag"] = mt.rank_diag()
    return out


def run_rows(accel_mod, w, P):
    """All the device work on the rows P of workload w, once: eval_batch's status at T = 1, model_explicit's rows, derive,
    push, and what check 4 compares of a table with every row pushed and of one with the accepted rows alone."""
    n = len(P)
    with open_acc(accel_mod, w) as acc:
        _, st_eval = acc.eval_batch(P, np.ones(n))
        own = [acc.model_explicit(p) for p in P]
        with accel_mod.ModeTable(acc, n) as mt, accel_mod.ModeTable(acc, n) as ref:
            cols = mt.columns()
            rows, st_d = mt.derive(P)
            st_p = mt.push(P)
            good = st_p == 0
            if good.any():
                ref.push(P[good])
            got, want = collect_all(mt), collect_all(ref)
    return dict(w=w, P=P, cols=cols, rows=rows, st_eval=st_eval, st_d=st_d, st_p=st_p, own=own, got=got, want=want)


def oracle_rows(w, P):
    """(status of the oracle's batch evaluation at T = 1 on y = 1, [(model row, its status)])"""
    mid, pl, x = w["model_case"], w["plength"], w["x"]
    _, rst = pyorc().generate_batch(mid, pl, x, np.ones(x.size), P, np.ones(len(P)))[:2]
    return np.asarray(rst), [pyorc().model(mid, p, pl, x) for p in P]


def special(accel_mod, mid, vi):
    if (mid, vi) not in RUNS:
        w = W.any_model(mid, Nx=3000, **VARIANTS[vi])
        cs = cases(mid, w)
        r = run_rows(accel_mod, w, np.stack([c[1] for c in cs]))
        r["names"], r["kinds"] = [c[0] for c in cs], [c[2] for c in cs]
        r["rst"], r["orc"] = oracle_rows(w, r["P"])
        RUNS[(mid, vi)] = r
    return RUNS[(mid, vi)]


def is_sum_overflow(r, k):
    """The header's one named exception to the status contract, "finite columns, overflowing sum": every column of the row
    finite, the oracle's model finite with status 0, every width's square finite (else the status rule itself rejects the
    row), and a width so large that a product of 2 l + 1 factors of the order Gamma^2 -- the eval kernels' common denominator
    of a multiplet's components -- leaves the double range."""
    cols, row = r["cols"], r["rows"][k]
    m_orc, st_orc = r["orc"][k]
    first = MR.first_columns(cols)
    with np.errstate(over="ignore"):
        g2 = row[first + 1] * row[first + 1]
        over = np.isinf(np.power(g2, 2.0 * cols["l"][first] + 1.0))
    return bool(np.all(np.isfinite(row)) and np.all(np.isfinite(g2)) and st_orc == 0 and r["rst"][k] == 0 and np.all(np.isfinite(m_orc))
                and over.any())


def check_status(r, tag):
    """Check 1.  Returns the mismatches [(tag, name, derive, push, eval, oracle)]."""
    bad = []
    for k, (name, kind) in enumerate(zip(r["names"], r["kinds"])):
        st = (int(r["st_d"][k]), int(r["st_p"][k]), int(r["st_eval"][k]), int(r["rst"][k]))
        print(f"status {tag} '{name}': derive {st[0]} push {st[1]} eval {st[2]} oracle {st[3]}")
        if is_sum_overflow(r, k):
            # asserted explicitly: the table accepts the row (and check 2 rebuilds the oracle's model from it), eval rejects it
            ok = st == (0, 0, 1, 0)
            if f"{tag} '{name}'" not in REPORT["exceptions"]:
                REPORT["exceptions"].append(f"{tag} '{name}'")
        elif kind == "overflow":
            ok = st == (1, 1, 1, 0)              # as the eval suite has it: the oracle's formula stays finite
        else:
            ok = st[0] == st[1] == st[2] == st[3]
        if not ok:
            bad.append((tag, name) + st)
    return bad


def expected_apart(mid, vi):
    """The case rows of (id, variant) that are not rebuilt, by name and in case order: (left out -- the oracle's status is
    not 0 or its row is not finite --, rejected -- the oracle's row is finite and the table rejects the row as eval_batch
    does: the eval suite's documented width overflow).  Found on the CPU oracle; pinned so that the set cannot drift."""
    if mid in (11, 14):
        return [], []
    if mid == 10:
        return ["W[0]<0"], []
    if mid == 9:
        return (["W[1]=W[0]", "W[0]<0"], []) if vi == 1 else (["W[0]<0"], ["W[1]=W[0]"] if vi == 0 else [])
    return ["f0==f1"], []


def check_reconstruction(r, tag, want_left_out=(), want_rejected=()):
    """Check 2.  Returns (worst ratio, rows rebuilt, rows left out, rows rejected beside a finite oracle row)."""
    w = r["w"]
    mid, pl, x = w["model_case"], w["plength"], w["x"]
    worst, rebuilt, left_out, rejected = 0.0, 0, [], []
    for k, name in enumerate(r["names"]):
        m_orc, st_orc = r["orc"][k]
        if np.any(np.isnan(m_orc)):
            assert r["st_d"][k] != 0 and r["st_eval"][k] != 0, (tag, name)
        if st_orc != 0 or r["rst"][k] != 0 or not np.all(np.isfinite(m_orc)):
            left_out.append(name)
            continue
        if r["st_d"][k] != 0:
            # the eval suite's documented exception (TAMCMC_CHAIN_NAN in tamcmc_accel.h): the oracle's row is finite, the row
            # is rejected here as by eval_batch, and there is no table row to rebuild a model from
            assert r["kinds"][k] == "overflow" and r["st_d"][k] == 1 and r["st_eval"][k] == 1, (tag, name, r["st_d"][k])
            rejected.append(name)
            continue
        m_own, st_own = r["own"][k]
        refs = [m_orc]
        if is_sum_overflow(r, k):
            assert st_own == 1 and np.any(np.isnan(m_own)), (tag, name)      # the library's own row overflowed: the oracle's alone
        else:
            assert st_own == 0, (tag, name)
            refs.append(m_own)
        R, S = MR.reconstruct(mid, pl, x, r["P"][k], r["rows"][k], r["cols"])
        for M in refs:
            ratio = MR.worst_ratio(R, S, M)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (tag, name, ratio)
        rebuilt += 1
    print(f"reconstruction {tag}: {rebuilt} rows rebuilt, left out {left_out}, rejected {rejected}, worst ratio {worst:.3g}")
    assert len(left_out) <= 2 and left_out == list(want_left_out) and rejected == list(want_rejected), (tag, left_out, rejected)
    return worst, rebuilt, len(left_out), len(rejected)


def inclination_ld(mid, pl, p):
    """The header's rule for the inclination column in long double: ids 2, 9, 10, 11 atan(p[s + 4] / p[s + 3]) in degrees, the
    quotient formed in double; ids 3, 6, 7, 8 the inclination entry as given; 0 elsewhere."""
    pl = [int(v) for v in pl]
    s, q = sum(pl[:6]), sum(pl[:9])
    if mid in ATAN_IDS:
        with np.errstate(all="ignore"):
            return np.arctan(LD(np.float64(p[s + 4]) / np.float64(p[s + 3]))) * 180 / PI_LD
    return LD(p[q]) if mid in GIVEN_IDS else LD(0)


def check_columns(r, tag):
    """Check 3 on the status-0 rows (the inclination rule on every row).  Returns the inclination's worst distance in ulps."""
    w, cols, P, rows = r["w"], r["cols"], r["P"], r["rows"]
    mid = w["model_case"]
    ok = np.flatnonzero(r["st_d"] == 0)
    amp = check_identities(w, cols, P[ok], rows[ok])
    assert amp <= 1, (tag, amp)
    worst = 0.0
    for k in range(len(P)):
        got, want = rows[k, K["inclination"]], inclination_ld(mid, w["plength"], P[k])
        if np.isnan(want):
            assert np.isnan(got) and r["st_d"][k] != 0, (tag, k)
            continue
        if mid in ATAN_IDS:
            assert -90.0 <= got <= 90.0, (tag, k, got)
            if want != 0:
                u = float(abs(LD(got) - want) / (ULP * abs(want)))
                worst = max(worst, u)
                assert u <= 4.0, (tag, k, got, want)
            else:
                assert got == 0.0, (tag, k, got)
        else:
            assert bits(got) == bits(np.float64(want)), (tag, k, got, want)       # as given (any quadrant), or +0
    l_of, kind = cols["l"], cols["kind"]
    split = kind == K["splitting"]
    nonneg = (kind == K["height"]) | (kind == K["h_m"]) | (kind == K["width"]) | split
    for k in ok:
        row = rows[k]
        assert np.all(bits(row[split & (l_of == 0)]) == bits(0.0)), (tag, k)
        assert np.all(row[nonneg] >= 0.0) and not np.any(np.signbit(row[nonneg])), (tag, k)
    return worst


def same_collection(got, want, tag):
    assert sorted(got) == sorted(want), (tag, sorted(got), sorted(want))
    for name in got:
        a, b = dict(got[name]), dict(want[name])
        if name == "result":
            a.pop("n_rejected"); b.pop("n_rejected")
        for key in a:                       # (scalars too: a NaN total equals a NaN total)
            a[key], b[key] = np.asarray(a[key]), np.asarray(b[key])
        try:
            same_results(a, b)
        except AssertionError as e:
            raise AssertionError(f"{tag}: {name}.{e}") from None


@pytest.mark.parametrize("mid", IDS)
def test_status_contract(accel_mod, mid):
    bad = []
    for vi, kw in enumerate(VARIANTS):
        bad += check_status(special(accel_mod, mid, vi), f"id {mid} {kw}")
    assert not bad, bad


SUM_OVERFLOW = {(10, 0): "W[0] tiny", (10, 1): "W[0] tiny", (10, 2): "W[0] tiny", (9, 2): "W[1]=W[0]"}


def test_the_named_exception(accel_mod):
    """The header's "finite columns, overflowing sum" by name.  'W[0] tiny' of id 10 in every variant: a reference frequency
    of 1e-6 in the AppWidth v2 width, Gamma ~ 5e37.  'W[1]=W[0]' of id 9 with do_amp: the exponent 2600 of the AppWidth v1
    width, where numax (weighted by the amplitudes) leaves the largest Gamma below 1.34e154, so that its square is finite
    -- without do_amp the same case squares to infinity and the table's own rule rejects it.  In each, eval_batch and
    model_explicit give TAMCMC_CHAIN_NAN, the oracle and the table TAMCMC_CHAIN_OK (and test_reconstruction rebuilds the oracle's
    row from the table's); no other case row is one."""
    for mid in IDS:
        for vi, kw in enumerate(VARIANTS):
            r = special(accel_mod, mid, vi)
            hits = [r["names"][k] for k in range(len(r["P"])) if is_sum_overflow(r, k)]
            assert hits == ([SUM_OVERFLOW[(mid, vi)]] if (mid, vi) in SUM_OVERFLOW else []), (mid, kw, hits)
            for name in hits:
                k = r["names"].index(name)
                st = (int(r["st_d"][k]), int(r["st_p"][k]), int(r["st_eval"][k]), int(r["rst"][k]), int(r["own"][k][1]))
                assert st == (0, 0, 1, 0, 1), (mid, kw, st)
                width = r["rows"][k][r["cols"]["kind"] == K["width"]]
                print(f"sum overflow id {mid} {kw} '{name}': widths {width.min():.3g} ... {width.max():.3g}")
                assert 1e31 < width.max() < 1.34e154, (mid, kw, width.max())


@pytest.mark.parametrize("mid", IDS)
def test_reconstruction(accel_mod, mid):
    worst = 0.0
    for vi, kw in enumerate(VARIANTS):
        r = special(accel_mod, mid, vi)
        ratio, rebuilt, left, rejected = check_reconstruction(r, f"id {mid} {kw}", *expected_apart(mid, vi))
        worst = max(worst, ratio)
        assert rebuilt + left + rejected == len(r["P"]) == (27 if mid in (11, 14) else 30)
        REPORT["rows"] += len(r["P"]); REPORT["rebuilt"] += rebuilt; REPORT["left_out"] += left; REPORT["not_rebuilt"] += rejected
    REPORT["ratio"][mid] = worst


def test_row_counts(accel_mod):
    """The totals of check 2 over every id and variant: 972 rows, 28 left out, 1 rejected beside a finite oracle row."""
    rows = left = rejected = 0
    for mid in IDS:
        for vi in range(len(VARIANTS)):
            r = special(accel_mod, mid, vi)
            want_left, want_rejected = expected_apart(mid, vi)
            apart = [name for k, name in enumerate(r["names"])
                     if r["orc"][k][1] != 0 or r["rst"][k] != 0 or not np.all(np.isfinite(r["orc"][k][0]))]
            assert apart == want_left, (mid, vi, apart)
            rows += len(r["P"]); left += len(want_left); rejected += len(want_rejected)
    assert (rows, left, rejected, rows - left - rejected) == (972, 28, 1, 943)


def test_amplitude_alone_a_nan(accel_mod):
    """The amplitude term of the status rule: id 11 with do_amp and a width of exactly 0 gives an infinite height (|A^2 / (pi 0)|)
    and amplitude = sqrt((pi inf) 0), a NaN, while every other column is a number.  The table, eval_batch, model_explicit and
    the oracle all reject the row."""
    w = W.any_model(11, Nx=3000, do_amp=True)
    off = np.concatenate([[0], np.cumsum(w["plength"])])
    P = np.tile(w["params_true"], (6, 1))
    P[1, off[7]] = 0.0
    r = run_rows(accel_mod, w, P)
    rst, orc = oracle_rows(w, P)
    row, cols = r["rows"][1], r["cols"]
    nan = np.isnan(row)
    assert nan.sum() == 1 and cols["kind"][nan][0] == K["amplitude"] and cols["mult"][nan][0] == 0, np.flatnonzero(nan)
    c0 = int(np.flatnonzero(nan)[0]) - 3
    assert row[c0 + 1] == 0.0 and np.isposinf(row[c0 + 2]) and np.isposinf(row[c0 + 7 + 1]), row[c0:c0 + 9]
    assert list(r["st_d"]) == list(r["st_p"]) == list(r["st_eval"]) == list(rst) == [0, 1, 0, 0, 0, 0], (r["st_d"], r["st_eval"], rst)
    assert r["own"][1][1] == 1 and r["got"]["result"]["n_rejected"] == 1
    same_collection(r["got"], r["want"], "amplitude alone")


@pytest.mark.parametrize("mid", IDS)
def test_identities_inclination_and_signs(accel_mod, mid):
    for vi, kw in enumerate(VARIANTS):
        REPORT["inc_ulp"] = max(REPORT["inc_ulp"], check_columns(special(accel_mod, mid, vi), f"id {mid} {kw}"))


@pytest.mark.parametrize("mid", IDS)
def test_rejected_rows_leave_no_trace(accel_mod, mid):
    for vi, kw in enumerate(VARIANTS):
        r = special(accel_mod, mid, vi)
        n_bad = int(np.count_nonzero(r["st_p"]))
        got, want = r["got"]["result"], r["want"]["result"]
        assert got["n_used"] == len(r["P"]) - n_bad == want["n_used"] and got["n_rejected"] == n_bad and want["n_rejected"] == 0
        assert got["n_used"] >= 4
        same_collection(r["got"], r["want"], f"id {mid} {kw}")
        REPORT["rejected"] += n_bad


def index_layout(accel_mod, mid, vi):
    """(run, tag) of the special rows the indices are checked on.  Id 2: the module's own layout.  Id 11: any_model's local
    layout holds two radial modes, fewer than the three an index plan needs -- the reference plan and enable_indices both refuse
    it, asserted here -- so the rows are the same cases of the local layout with four radial modes (workloads.local_asymptotic)."""
    if mid != 11:
        return special(accel_mod, mid, vi)
    if ("index", vi) not in RUNS:
        r = special(accel_mod, 11, vi)
        ok = int(np.flatnonzero(r["st_d"] == 0)[0])
        with pytest.raises(SR.Refused):
            SR.plan(r["cols"], r["rows"][ok])
        with open_acc(accel_mod, r["w"]) as acc, accel_mod.ModeTable(acc, 4) as mt:
            with pytest.raises(accel_mod.AccelError) as e:
                mt.enable_indices(r["w"]["params_true"])
            assert e.value.code == accel_mod.capi.E_INVALID
        w = W.local_asymptotic(**VARIANTS[vi])
        cs = cases(11, w)
        r = run_rows(accel_mod, w, np.stack([c[1] for c in cs]))
        r["names"], r["kinds"] = [c[0] for c in cs], [c[2] for c in cs]
        r["rst"], r["orc"] = oracle_rows(w, r["P"])
        RUNS[("index", vi)] = r
    return RUNS[("index", vi)]


@pytest.mark.parametrize("mid", [2, 11])
def test_indices_of_the_special_rows(accel_mod, mid):
    """Check 5 (and, for the second local layout, checks 1 to 3 again)."""
    for vi, kw in enumerate(VARIANTS):
        r = index_layout(accel_mod, mid, vi)
        if mid == 11:
            tag = f"id 11, four radial modes, {kw}"
            assert not check_status(r, tag)
            check_reconstruction(r, tag)
            check_columns(r, tag)
        w, P, nb = r["w"], r["P"], len(r["cols"])
        with open_acc(accel_mod, w) as acc, accel_mod.ModeTable(acc, len(P)) as mt:
            ref, st_ref = mt.derive(w["params_true"][None, :])
            assert st_ref[0] == 0
            plan = SR.plan(r["cols"], ref[0])
            info = mt.enable_indices(w["params_true"])
            assert info["n_base_cols"] == nb and info["n_index_cols"] == len(plan["terms"]) > 0
            rows, st = mt.derive(P)
            st_p = mt.push(P)
        assert np.array_equal(bits(rows[:, :nb]), bits(r["rows"])), (mid, kw)
        with np.errstate(all="ignore"):
            want = SR.evaluate(plan["terms"], rows[:, :nb])
        assert np.array_equal(bits(rows[:, nb:]), bits(want)), (mid, kw, np.argwhere(bits(rows[:, nb:]) != bits(want))[:5])
        nan_index = np.isnan(rows[:, nb:]).any(axis=1)
        expect = np.where(r["st_d"] != 0, r["st_d"], nan_index.astype(np.int32))
        assert np.array_equal(st, expect) and np.array_equal(st_p, expect), (mid, kw, st, expect)
        accepted_inf = (st == 0) & np.isinf(rows[:, nb:]).any(axis=1)
        print(f"indices id {mid} {kw}: accepted with an infinite index {[r['names'][k] for k in np.flatnonzero(accepted_inf)]}, "
              f"rejected for a NaN index {[r['names'][k] for k in np.flatnonzero((r['st_d'] == 0) & nan_index)]}")
        REPORT["inf_index"] += int(accepted_inf.sum())
        REPORT["nan_index"] += int(((r["st_d"] == 0) & nan_index).sum())


def reference_setups(tmp_path):
    for k in range(len(model_file_slices(MODEL))):
        yield f"TF slice {k}", Setup(CFG).load(MODEL, DATA, k), 10 + k
    for name, reader in REF_MODEL_FILES:
        yield name, load_on_flat_spectrum(name, reader, tmp_path), 21


def test_reference_inputs(accel_mod, tmp_path):
    """Check 6."""
    worst = 0.0
    for tag, s, seed in reference_setups(tmp_path):
        w = dict(model_case=s.model_case, plength=np.asarray(s.plength, dtype=np.int32), x=s.x)
        P = chains_around(s, 4, seed=seed)
        r = run_rows(accel_mod, w, P)
        r["names"], r["kinds"] = [f"row {k}" for k in range(4)], [None] * 4
        r["rst"], r["orc"] = oracle_rows(w, P)
        assert not check_status(r, tag)
        ratio = check_reconstruction(r, tag)[0]
        worst = max(worst, ratio)
        REPORT["inc_ulp"] = max(REPORT["inc_ulp"], check_columns(r, tag))
    REPORT["ratio"]["files"] = worst


def test_zz_report():
    """Not a check: the lines DESIGN.md quotes (run after the cases of this module)."""
    if REPORT["ratio"]:
        print("modetable special worst |R - M| / bound: " + ", ".join(f"{k}: {v:.3g}" for k, v in REPORT["ratio"].items()))
        print(f"modetable special: {REPORT['rebuilt']} of {REPORT['rows']} rows rebuilt, {REPORT['left_out']} left out, "
              f"{REPORT['not_rebuilt']} rejected beside a finite oracle row, "
              f"exceptions {REPORT['exceptions']}; {REPORT['rejected']} rows rejected; inclination within {REPORT['inc_ulp']:.3g} ulp; "
              f"{REPORT['inf_index']} accepted rows with an infinite index, {REPORT['nan_index']} rejected for a NaN index")
