"""fitcompare_hip on the GPU: two small files in chainsummary_hip's format (the --loo output file, and the .loowin file) written
by the test; the totals, counts and weights in the result file's header parse back (17 digits) to the numbers of the Python
object on the same parsed values; the rows hold the leading columns and d_1 ... d_{K-1}; <result file>.top lists the units of
largest |d|; files that do not belong together are refused with a non-zero exit."""
import os
import subprocess

import numpy as np
import pytest

from support import ROOT, bits, tool

pytestmark = pytest.mark.gpu


def exe():
    tool()
    return os.path.join(ROOT, "bin", "fitcompare_hip")


def write_loo(path, x, y, elpd, khat):
    with open(path, "w") as f:
        f.write("# chainsummary_hip (test)\n# n_used= 50  n_rejected= 0\n# x y mean_M sd_M min_M max_M lppd var_l elpd_loo pareto_k\n")
        for i in range(x.size):
            f.write("%.10f %.12g 1 0.1 0.9 1.1 -1 0.01 %.12g %.12g\n" % (x[i], y[i], elpd[i], khat[i]))


def write_loowin(path, first, last, elpd, khat):
    with open(path, "w") as f:
        f.write("# chainsummary_hip (test)\n# W= 20  first= 20  n_windows= %d\n" % first.size)
        f.write("# first_bin last_bin x_first x_last elpd_lwo pareto_k tail_len\n")
        for i in range(first.size):
            f.write("%d %d %.12g %.12g %.12g %.12g 12\n" % (first[i], last[i], 0.01 * first[i], 0.01 * last[i], elpd[i], khat[i]))


def header(path):
    out = {}
    for line in open(path):
        if not line.startswith("#"):
            break
        t = line[1:].split()
        if t and t[0] in ("pair", "prob"):
            vals = dict(zip(t[3::2], t[4::2]))
            out[(t[0], int(t[1]), int(t[2]))] = {k.rstrip("="): float(v) for k, v in vals.items()}
        elif t and t[0].endswith("=") and t[0][:-1] in ("pseudo_bma", "pseudo_bma_plus", "stacking"):
            out[t[0][:-1]] = np.array([float(v) for v in t[1:]])
        elif t and t[0] in ("stacking_info", "bootstrap"):
            out[t[0]] = {k.rstrip("="): float(v) for k, v in zip(t[1::2], t[2::2])}
        elif t and t[0] == "fits=":
            out["fits"] = dict(zip([k.rstrip("=") for k in t[0::2]], t[1::2]))
    return out


def parsed(values):
    """what the tool reads back from %.12g"""
    return np.array([float("%.12g" % v) for v in values])


def test_tool_against_the_python_object(accel_mod, tmp_path):
    rng = np.random.default_rng(11)
    N, K = 300, 3
    x = 2300.0 + 0.0084 * np.arange(N)
    y = rng.exponential(size=N)
    elpd = rng.normal(-2.0, 1.0, N)[None, :] + 0.2 * rng.standard_normal((K, N)) - 0.05 * np.arange(K)[:, None]
    kh = rng.uniform(0.0, 1.0, (K, N))
    elpd[1, 17], kh[2, 40] = np.nan, np.inf
    files = [str(tmp_path / ("fit%d.txt" % k)) for k in range(K)]
    for k in range(K):
        write_loo(files[k], x, y, elpd[k], kh[k])
    out = str(tmp_path / "cmp.txt")
    r = subprocess.run([exe()] + files + [out, "--bootstrap", "300,7", "--stacking", "1e-9,20000", "--scale", "0.5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    h = header(out)
    e, k_ = np.stack([parsed(v) for v in elpd]), np.stack([parsed(v) for v in kh])
    assert h["fits"]["fits"] == "3" and h["fits"]["units"] == "300" and h["fits"]["n_included"] == "299" and h["fits"]["column"] == "elpd_loo"
    with accel_mod.Compare(e, k_, scale=0.5, seed=7) as cmp:
        cmp.bootstrap(300)
        st = cmp.stacking(1e-9, 20000)
        for a in range(1, K):
            for b in range(a):
                d, got = cmp.diff(a, b), h[("pair", a, b)]
                for key in ("elpd_diff", "se_diff", "n_better", "n_worse", "n_k_high", "diff_k_high"):
                    assert np.array_equal(bits(got[key]), bits(float(d[key]))), (a, b, key)
                gt, eq, R = cmp.prob(a, b)
                p = h[("prob", a, b)]
                assert (p["n_greater"], p["n_equal"]) == (gt, eq) and R == 300
                assert p["q05"] == cmp.interval(a, b, 0.05) and p["q95"] == cmp.interval(a, b, 0.95)
        for m in ("pseudo_bma", "pseudo_bma_plus", "stacking"):
            assert np.array_equal(bits(h[m]), bits(cmp.weights(m))), m
        info = h["stacking_info"]
        assert (info["iterations"], info["converged"]) == (st["iterations"], st["converged"]) and info["gap"] == st["gap"] and info["f"] == st["f"]
        assert h["bootstrap"] == dict(R=300.0, seed=7.0)
    rows = np.loadtxt(out)
    assert rows.shape == (N, 2 + K - 1) and np.array_equal(rows[:, 0], np.array([float("%.10f" % v) for v in x]))
    for k in range(1, K):
        assert np.array_equal(bits(rows[:, 1 + k]), bits(e[k] - e[0]))
    top = np.loadtxt(out + ".top")
    assert top.shape == (20 * (K - 1), 5)
    for k in range(1, K):
        mine = top[top[:, 0] == k]
        d = np.where(np.isfinite(e).all(axis=0), np.abs(e[k] - e[0]), -1.0)
        assert np.array_equal(mine[:, 1].astype(int), np.argsort(-d, kind="stable")[:20]) and np.all(np.diff(np.abs(mine[:, 4])) <= 0)


def test_tool_reads_window_files_and_refuses_mismatches(accel_mod, tmp_path):
    rng = np.random.default_rng(12)
    n = 40
    first = 20 * np.arange(n)
    last = first + 19
    elpd = rng.normal(-30.0, 3.0, (2, n))
    kh = rng.uniform(0.0, 0.6, (2, n))
    a, b, c, d = (str(tmp_path / s) for s in ("a.loowin", "b.loowin", "c.loowin", "d.loowin"))
    write_loowin(a, first, last, elpd[0], kh[0])
    write_loowin(b, first, last, elpd[1], kh[1])
    write_loowin(c, first[:-1], last[:-1], elpd[1][:-1], kh[1][:-1])
    write_loowin(d, first + 1, last + 1, elpd[1], kh[1])
    out = str(tmp_path / "w.txt")
    r = subprocess.run([exe(), a, b, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    h = header(out)
    assert h["fits"]["column"] == "elpd_lwo" and "stacking" not in h and "pseudo_bma_plus" not in h
    with accel_mod.Compare(np.stack([parsed(elpd[0]), parsed(elpd[1])]), np.stack([parsed(kh[0]), parsed(kh[1])])) as cmp:
        assert h[("pair", 1, 0)]["elpd_diff"] == cmp.diff(1, 0)["elpd_diff"] and h[("pair", 1, 0)]["se_diff"] == cmp.diff(1, 0)["se_diff"]
        assert np.array_equal(bits(h["pseudo_bma"]), bits(cmp.weights("pseudo_bma")))
    rows = np.loadtxt(out)
    assert rows.shape == (n, 3) and np.array_equal(rows[:, 0], first) and np.array_equal(rows[:, 1], last)
    for other, why in ((c, "rows"), (d, "leading columns")):
        bad = str(tmp_path / "bad.txt")
        r = subprocess.run([exe(), a, other, bad, "--bootstrap", "10"], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and why in r.stderr and not os.path.exists(bad), (other, r.stderr)
